"""The layer of the reflow / diffusion-fast denoiser (``NaiveV2DiffLayer`` of ``reflow.naive_v2_diff``, the same text in
``diffusion.naive_v2_diff``) on HIP: csrc/naive_v2_layer.h, two launches per layer call -- the step bias, the condition projection,
the first pointwise convolution and the GLU; then the 31-tap depthwise convolution, the SiLU, the second pointwise convolution
and the residual -- with the GLU's output handed over through a workspace.  f32 MFMA.

  tile                        ``(t_A, t_B)``: frames per workgroup of the two launches (``ddsp_hip_naive_v2_layer_tile``)
  diff_layer                  the functional form: ``x [B, L, D]``, ``cond [B, L, Hc]``, ``d [B, D]``, the eight weight tensors
  choose_form                 ``"split"``, ``"tiled"`` or None (torch) for a size, from the two measured tables
  diff_stack                  all layers of a denoiser: one matmul for every layer's step projection, one launch pair per layer
  layer_forward / net_forward the dispatchers bound as ``NaiveV2DiffLayer.forward`` / ``NaiveV2Diff.forward``
  patch_reference_naive_v2    rebinds those two in whichever of the two reference modules import; opt-in
  unpatch_reference_naive_v2
  release_workspace           drop the cached workspaces

Dispatch (``layer_eligible``) is decided from a module's structure, not its class: ``attn is None``, ``wavenet_like_proj is
None``, a ``conformer`` that is the conv chain of ``conformer._conv_spec`` without LayerNorm and with an inactive dropout, a
``diffusion_step_projection`` ``Conv1d(D, D, 1)`` and a ``condition_projection`` ``Conv1d(Hc, D, 1)``, plain float32 parameters
without hooks and none of them an inference tensor, float32 tensors on the GPU, no gradient needed, autocast off, (D, Hc) =
(512, 128).  Everything else runs the
module's own forward.  ``LAYER_TORCH_FASTER`` maps D to the number of frames B L below which the same-GPU torch chain was
measured faster (tools/naive_v2_bench.py); None: at every size, which is also what a D without a committed
measurement gets.

The layer has a second form, csrc/naive_v2_split.h (``form="split"``): the same sums in the same order, hence the same bits, with
a frame tile of 16 and the channels split over workgroups, four launches, for calls of a few hundred frames (``B ceil(L / 16) <=
4096``).  ``SPLIT_BELOW`` maps D to the number of frames below which it was measured the fastest of the three, and
``choose_form`` is the one place where the hook decides between the split form, the tiled form and torch.
"""
import collections

import torch
import torch.nn.functional as F

from . import _ffi, _modules
from . import conformer as _conformer
from ._modules import (FORMS, SPLIT_MAX_TILES, autocast_on, drop_workspaces, needs_grad, on_device, pack_host, packed_table,
                       pointwise, step_biases, stream_workspace)
from ._patching import patch_forwards, run_reference, unpatch_forwards

SHAPES = ((512, 128),)
TAPS = 31
# D -> the number of frames B L below which the torch op chain was measured faster on the same GPU (None: at every size; the
# hook then routes nothing for that D, the functional API still runs the kernels).  tools/naive_v2_bench.py on one MI355X
# (profiles/naive_v2_throughput.json, naive_v2_latency.json): torch is faster at 1 x 100, 1 x 203 and 48 x 172 = 8 256 frames
# (x0.23, x0.23, x0.87), the kernels at 32 x 862 = 27 584, the smallest size at which they were seen to win (x1.62), and at
# 64 x 862 (x1.68).
LAYER_TORCH_FASTER = {512: 27584}
# D -> the number of frames B L below which the channel-split form (csrc/naive_v2_split.h) was MEASURED faster than both the
# torch chain and the tiled form (tools/naive_v2_bench.py --mode split, profiles/naive_v2_split_latency.json): the smallest
# measured size at which it was not the fastest of the three; no entry where it is not the fastest at 1 x 100.  On one MI355X it
# was the fastest at all five measured sizes -- 1 x 100, 1 x 203, 4 x 203, 1 x 862 (x1.88, x1.67, x1.32, x1.51 over torch) and, by
# 3 %, 48 x 172 = 8 256 frames --, so the bound is one past the largest of them: nothing above it was measured.
SPLIT_BELOW = {512: 8257}
# dispatch counters (tests and tools read them): layer calls ("hip": on the kernels in either form, "split": those of them that
# took the split form); separate from conformer.CALLS and wavenet.CALLS
CALLS = {"hip": 0, "reference": 0, "split": 0}
PACKS = {"count": 0}                                   # weight tables built (a cache hit does not count)
_WS = collections.OrderedDict()                        # (device, stream) -> the buffer the GLU's output passes through
_WS_MAX = 16


def tile(D, Hc):
    """``(t_A, t_B)``: frames per workgroup of the first and the second launch; ``(0, 0)`` for a shape the kernels do not take"""
    lib = _ffi.lib()
    return int(lib.ddsp_hip_naive_v2_layer_tile(int(D), int(Hc), 0)), int(lib.ddsp_hip_naive_v2_layer_tile(int(D), int(Hc), 1))


def split_tile(D, Hc):
    """frames per workgroup of the split form; 0 for a shape the kernels do not take"""
    return int(_ffi.lib().ddsp_hip_naive_v2_layer_split_tile(int(D), int(Hc)))


def split_in_range(B, L):
    """the split form takes ``B ceil(L / 16)`` tiles up to ``SPLIT_MAX_TILES`` (``_modules.split_in_range``)"""
    return _modules.split_in_range(B, L)


def choose_form(D, B, L):
    """where the hook sends a layer call of ``B x L`` frames: ``"split"`` within the split form's range below the measured
    ``SPLIT_BELOW[D]``, else ``"tiled"`` unless ``LAYER_TORCH_FASTER`` gives the size to torch, else None (the torch chain):
    ``_modules.choose_form`` on this module's two tables as they are now"""
    return _modules.choose_form(SPLIT_BELOW, LAYER_TORCH_FASTER, D, B, L)


def _workspace(B, L, D, x, form="tiled"):
    """the buffer the intermediates pass through (tiled: the GLU's output; split: x', the GLU's output and the stencil's), for
    ``x``'s device and the caller's stream there (``_modules.stream_workspace``'s rule)"""
    lib = _ffi.lib()
    size = lib.ddsp_hip_naive_v2_layer_split_workspace_bytes if form == "split" else lib.ddsp_hip_naive_v2_layer_workspace_bytes
    return stream_workspace(_WS, max(int(size(B, L, D)) // 4, 4), x, _WS_MAX)


def release_workspace():
    """drop the cached hand-over buffers of every device and stream"""
    drop_workspaces(_WS)


def _pack(dims, flat):
    """the host table of ``(wc, bc, w1, b1, wd, bd, w2, b2)``, for ``packed_table``"""
    lib = _ffi.lib()
    refusal = "diff_layer: (D, Hc) = (%d, %d) is outside the kernels' range" % dims
    host = pack_host(int(lib.ddsp_hip_naive_v2_layer_pack_bytes(*dims)), refusal, flat, lib.ddsp_hip_naive_v2_layer_pack, dims)
    PACKS["count"] += 1
    return host


def _check_weights(weights, D, Hc):
    if len(weights) != 8:
        raise ValueError("diff_layer: weights must be (wc, bc, w1, b1, wd, bd, w2, b2)")
    want = ((D, Hc, 1), (D,), (4 * D, D, 1), (4 * D,), (2 * D, 1, TAPS), (2 * D,), (D, 2 * D, 1), (D,))
    if any(tuple(t.shape) != s or t.dtype != torch.float32 for t, s in zip(weights, want)):
        raise ValueError("diff_layer: weights must be float32 [D, Hc, 1], [D], [4 D, D, 1], [4 D], [2 D, 1, 31], [2 D], "
                         "[D, 2 D, 1], [D]")


def diff_layer(x, cond, d, weights, out=None, ws=None, form="tiled"):
    """One layer on the HIP kernels: ``x [B, L, D]``, ``cond [B, L, Hc]`` (a frame's channels contiguous), ``d [B, D]`` (the
    layer's projection of the step embedding), ``weights = (wc [D, Hc, 1], bc [D], w1 [4 D, D, 1], b1 [4 D], wd [2 D, 1, 31],
    bd [2 D], w2 [D, 2 D, 1], b2 [D])``, all float32.  Returns ``x + conv_module(x + d + Wc cond + bc)`` in ``out``, which must not
    be ``x``.  ``form``: ``"tiled"`` (csrc/naive_v2_layer.h, two launches) or ``"split"`` (csrc/naive_v2_split.h, four launches with
    a frame tile of 16 for calls of a few hundred frames, ``B ceil(L / 16) <= 4096``, ValueError beyond); both give the same bits.
    ``ws``: a float32 buffer of at least ``B 2 D L`` (tiled) or ``5 B L D`` (split) elements for the intermediates, instead of the
    cached one of the caller's stream.  No synchronisation; once the weight table and the workspace exist the only allocation is
    the result (when ``out`` is None), so a call can be captured in a graph (a capture without ``ws`` takes a workspace from the
    graph's pool)."""
    _ffi.check_device(x, cond, d, out)
    if any(not isinstance(t, torch.Tensor) or t.dtype != torch.float32 for t in (x, cond, d)) or x.dim() != 3 or cond.dim() != 3:
        raise ValueError("diff_layer: x [B, L, D], cond [B, L, Hc] and d [B, D] must be float32 tensors")
    B, L, D = x.shape
    Hc = cond.shape[2]
    if (D, Hc) not in SHAPES:
        raise ValueError("diff_layer: (D, Hc) = (%d, %d) is outside the kernels' range" % (D, Hc))
    if cond.shape[0] != B or cond.shape[1] != L or tuple(d.shape) != (B, D):
        raise ValueError("diff_layer: cond must be [B, L, Hc] and d [B, D]")
    _check_weights(weights, D, Hc)
    if L < 1:
        raise ValueError("diff_layer: L must be positive")
    if form not in FORMS:
        raise ValueError("diff_layer: form must be 'tiled' or 'split'")
    if form == "split" and not _modules.split_in_range(B, L):
        raise ValueError("diff_layer: the split form takes B ceil(L / 16) <= %d tiles" % SPLIT_MAX_TILES)
    if out is x or out is cond:
        raise ValueError("diff_layer: out must be neither x nor cond")
    x, cond, d = x.contiguous(), cond.contiguous(), d.contiguous()
    y = torch.empty_like(x) if out is None else out
    if not y.is_contiguous() or y.shape != x.shape or y.dtype != torch.float32:
        raise ValueError("diff_layer: out must be a contiguous float32 tensor of x's shape")
    if B == 0:
        return y
    lib = _ffi.lib()
    table = packed_table("naive_v2", (D, Hc), list(weights), x.device, _pack)
    if ws is None:
        ws = _workspace(B, L, D, x, form)
    elif ws.dtype != torch.float32 or not ws.is_contiguous() or ws.device != x.device:
        raise ValueError("diff_layer: ws must be a contiguous float32 tensor on x's device")
    CALLS["hip"] += 1
    if form == "split":
        CALLS["split"] += 1
    entry = lib.ddsp_hip_naive_v2_layer_split if form == "split" else lib.ddsp_hip_naive_v2_layer
    _ffi.check(entry(x.data_ptr(), cond.data_ptr(), d.data_ptr(), y.data_ptr(), table.data_ptr(), table.numel() * 4, ws.data_ptr(),
                     ws.numel() * 4, B, L, D, Hc, _ffi.stream_of(x)))
    return y


def diff_stack(x, cond, s, layers, form="tiled"):
    """The layers of a denoiser: ``x [B, L, D]``, ``cond [B, L, Hc]``, ``s [B, D]`` (the step embedding), ``layers`` a list of
    ``(weights, (wp [D, D, 1], bp [D]))``.  The step projections of all layers are ONE matmul; then one launch pair per layer, x
    handed over through two buffers (the caller's x is never written), one workspace for all layers (in a graph capture as
    well).  ``form`` as in ``diff_layer``, for every layer.  Returns x after the last layer."""
    if not layers:
        raise ValueError("diff_stack: no layers")
    if any(not isinstance(t, torch.Tensor) or t.dtype != torch.float32 for t in (x, s)) or x.dim() != 3 or x.shape[1] < 1:
        raise ValueError("diff_stack: x [B, L, D] and s [B, D] must be float32 tensors, L positive")
    B, L, D = x.shape
    n = len(layers)
    if tuple(s.shape) != (B, D) or any(tuple(p[0].shape) != (D, D, 1) or tuple(p[1].shape) != (D,) for _, p in layers):
        raise ValueError("diff_stack: s must be [B, D] and every step projection ([D, D, 1], [D])")
    if form not in FORMS or (form == "split" and not _modules.split_in_range(B, L)):
        raise ValueError("diff_stack: form must be 'tiled' or 'split', the latter with B ceil(L / 16) <= %d" % SPLIT_MAX_TILES)
    _ffi.check_device(x, cond, s)
    d = step_biases(s, [p for _, p in layers])                                            # [n, B, D]
    cond = cond.contiguous()
    bufs = (torch.empty_like(x, memory_format=torch.contiguous_format),
            torch.empty_like(x, memory_format=torch.contiguous_format) if n > 1 else None)
    ws = _workspace(B, L, D, x, form) if B else None
    src = x
    for i, (weights, _) in enumerate(layers):
        dst = bufs[(n - 1 - i) % 2]                    # the last layer writes the first buffer
        diff_layer(src, cond, d[i], weights, out=dst, ws=ws, form=form)
        src = dst
    return src


# ---- the reference's modules --------------------------------------------------------------------------------------------------

def _layer_spec(layer):
    """``(weights, (wp, bp))`` of a module with the layer's submodules in the kernels' form, or None"""
    if not isinstance(layer, torch.nn.Module) or layer._forward_pre_hooks or layer._forward_hooks:
        return None
    if getattr(layer, "attn", True) is not None or getattr(layer, "wavenet_like_proj", True) is not None:
        return None
    conv = getattr(layer, "conformer", None)
    sp, cp = getattr(layer, "diffusion_step_projection", None), getattr(layer, "condition_projection", None)
    if not isinstance(conv, torch.nn.Module) or not isinstance(cp, torch.nn.Conv1d):
        return None
    spec = _conformer._conv_spec(conv)
    if spec is None:
        return None
    cw, norm, _, drop = spec
    if norm is not None or (drop.p != 0 and drop.training):
        return None
    D, Hc = cw[0].shape[1], cp.in_channels
    if not pointwise(sp, D, D) or not pointwise(cp, Hc, D):
        return None
    return (cp.weight, cp.bias) + tuple(cw), (sp.weight, sp.bias)


def layer_eligible(layer, x, cond, step):
    """the ``(weights, (wp, bp))`` to run ``layer`` on the reference's ``x [B, D, L]``, ``cond [B, Hc, L]``, ``step [B, D, 1]``
    with the HIP kernels (in the form ``choose_form`` names for the size), or None: the layer's own forward"""
    if not on_device(x, 3) or not on_device(cond, 3) or not on_device(step, 3) or x.shape[2] < 1:
        return None
    if autocast_on(x):
        return None
    spec = _layer_spec(layer)
    if spec is None:
        return None
    weights, proj = spec
    D, Hc = weights[2].shape[1], weights[0].shape[1]
    B, L = x.shape[0], x.shape[2]
    if (D, Hc) not in SHAPES or x.shape[1] != D or tuple(cond.shape) != (B, Hc, L) or tuple(step.shape) != (B, D, 1):
        return None
    flat = list(weights) + list(proj)
    if any(t.device != x.device for t in flat + [cond, step]) or needs_grad([x, cond, step] + flat):
        return None
    if choose_form(D, B, L) is None:
        return None
    return spec


def _reference_layer_forward(layer, x, condition, diffusion_step):
    CALLS["reference"] += 1
    return run_reference(layer, getattr(layer, "reference_forward", None), x, condition, diffusion_step)


def layer_forward(layer, x, condition=None, diffusion_step=None):
    """the dispatcher bound as ``NaiveV2DiffLayer.forward``: ``[B, D, L]`` in any strides in (a transposed view of a contiguous
    ``[B, L, D]`` costs no copy); returns ``y.transpose(1, 2)``, a ``[B, D, L]`` view of the contiguous ``[B, L, D]`` result"""
    spec = None
    if isinstance(x, torch.Tensor) and isinstance(condition, torch.Tensor) and isinstance(diffusion_step, torch.Tensor):
        spec = layer_eligible(layer, x, condition, diffusion_step)
    if spec is None:
        return _reference_layer_forward(layer, x, condition, diffusion_step)
    weights, (wp, bp) = spec
    d = torch.addmm(bp, diffusion_step[:, :, 0], wp[:, :, 0].t())
    form = choose_form(x.shape[1], x.shape[0], x.shape[2])
    return diff_layer(x.transpose(1, 2), condition.transpose(1, 2), d, weights, form=form).transpose(1, 2)


def _stack_candidate(net, spec, cond):
    """what can be told before anything is computed: a float32 mel ``[B, M, L]`` or ``[B, 1, M, L]`` and a condition on the GPU,
    no condition masking, not wavenet_like, every layer in the kernels' form, no gradient through the net, a size the kernels
    are routed at"""
    layers = list(net.residual_layers)
    if not layers or net.mask_cond_ratio is not None or getattr(net, "wavenet_like", False):
        return False
    if not (on_device(spec, 3) or on_device(spec, 4)) or not on_device(cond, 3) or autocast_on(spec):
        return False
    specs = [_layer_spec(layer) for layer in layers]
    if any(sp is None for sp in specs) or needs_grad([spec, cond] + list(net.parameters())):
        return False
    return choose_form(specs[0][0][2].shape[1], spec.shape[0], spec.shape[-1]) is not None


def net_forward(net, spec, diffusion_step, cond):
    """the dispatcher bound as ``NaiveV2Diff.forward``.  When every layer can run on the kernels: the module's own
    ``input_projection`` + GELU, ``diffusion_embedding``, ``conditioner_projection`` and ``output_projection`` around
    ``diff_stack``, x and the condition transposed once per call, a mel that came with a singleton axis 1 gets it back.
    Everything else -- condition masking, wavenet_like, an ineligible layer or tensor -- is the module's own forward, whose
    layers then dispatch one by one."""
    if _stack_candidate(net, spec, cond):
        mel = spec.select(1, 0) if spec.dim() == 4 else spec
        x = F.gelu(net.input_projection(mel))
        step = net.diffusion_embedding(diffusion_step).unsqueeze(-1)
        condition = net.conditioner_projection(cond)
        specs = [layer_eligible(layer, x, condition, step) for layer in net.residual_layers]
        if all(sp is not None for sp in specs):
            form = choose_form(x.shape[1], x.shape[0], x.shape[2])
            y = diff_stack(x.transpose(1, 2), condition.transpose(1, 2), step.select(2, 0), specs, form)
            out = net.output_projection(y.transpose(1, 2))
            return out.unsqueeze(1) if spec.dim() == 4 else out
    return run_reference(net, getattr(net, "reference_forward", None), spec, diffusion_step, cond)


_REFERENCE_MODULES = ("diffusion.naive_v2_diff", "reflow.naive_v2_diff")


_CLASSES = (("NaiveV2DiffLayer", lambda self, x, condition=None, diffusion_step=None:
             layer_forward(self, x, condition, diffusion_step)),
            ("NaiveV2Diff", lambda self, spec, diffusion_step, cond: net_forward(self, spec, diffusion_step, cond)))


def patch_reference_naive_v2():
    """Route ``NaiveV2DiffLayer.forward`` and ``NaiveV2Diff.forward`` of whichever of ``diffusion.naive_v2_diff`` and
    ``reflow.naive_v2_diff`` import through the dispatchers above.  Idempotent; returns the list of modules patched.
    ``vocoder.patch_reference()`` does not call it, and it leaves ``patch_reference_conformer`` alone: the hook is opt-in, and a
    layer that runs on the kernels never reaches its inner conv module."""
    return patch_forwards(_REFERENCE_MODULES, _CLASSES)


def unpatch_reference_naive_v2():
    """Undo ``patch_reference_naive_v2()``."""
    unpatch_forwards(_REFERENCE_MODULES, [name for name, _ in _CLASSES])
