"""The residual layer of the diffusion denoiser's WaveNet (``ResidualBlock`` of ``diffusion.wavenet``) on HIP:
csrc/wavenet_layer.h, one launch per layer call, the 3-tap convolution with the conditioner projection and the output projection
as f32 MFMA GEMMs, the gate between them on the CU, the skip sum accumulated in place.

  tile                        frames per workgroup (``ddsp_hip_wavenet_layer_tile``)
  residual_layer              the functional form: ``x [B, C, T]``, ``cond [B, H, T]``, ``d [B, C]``, ``(wdil, bdil, wc, bc, wo, bo)``
  choose_form                 ``"split"``, ``"tiled"`` or None (torch) for a size, from the two measured tables
  residual_stack              all layers of a WaveNet: one matmul for every layer's step projection, one launch per layer
  layer_forward / net_forward the dispatchers bound as ``ResidualBlock.forward`` / ``WaveNet.forward``
  patch_reference_wavenet     rebinds those two in ``diffusion.wavenet``; opt-in (``patch_reference`` leaves it)
  unpatch_reference_wavenet

Dispatch (``layer_eligible``) is decided from a module's structure, not its class: a ``dilated_conv`` ``Conv1d(C, 2 C, 3,
padding 1, dilation 1)`` with zeros padding, a ``conditioner_projection`` ``Conv1d(H, 2 C, 1)``, an ``output_projection``
``Conv1d(C, 2 C, 1)`` and a ``diffusion_projection`` ``Linear(C, C)``, plain float32 parameters without hooks, float32 tensors on
the GPU, no gradient needed, autocast off, no parameter an inference tensor, (C, H) = (384, 256) or (512, 256).  Everything else runs the module's own forward.
``LAYER_TORCH_FASTER`` maps C to the number of frames B T below which the same-GPU torch chain was measured faster
(tools/wavenet_bench.py); None: at every size, which is also what a C without a committed measurement gets.

The layer has a second form, csrc/wavenet_split.h (``form="split"``): the same sums in the same order, hence the same bits, with a
frame tile of 16 and the channels split over workgroups, two launches (the gate into a workspace, then the output projection),
for calls of a few hundred frames (``B ceil(T / 16) <= 4096``).  ``SPLIT_BELOW`` maps C to the number of frames below which it was
measured the fastest of the three, and ``choose_form`` is the one place where the hook decides between the split form, the tiled
form and torch.
"""
import collections
import math

import torch

from . import _ffi, _modules
from ._modules import (FORMS, SPLIT_MAX_TILES, autocast_on, drop_workspaces, needs_grad, on_device, pack_host, packed_table,
                       pad_of, plain_with_bias, step_biases, stream_workspace)
from ._patching import patch_forwards, run_reference, unpatch_forwards

SHAPES = ((384, 256), (512, 256))
# C -> the number of frames B T below which the torch op chain was measured faster on the same GPU (None: at every size; the
# hook then routes nothing for that C, the functional API still runs the kernel).  tools/wavenet_bench.py on one MI355X
# (profiles/wavenet_throughput.json, wavenet_latency.json): at both C torch is faster at 1 x 100, 1 x 203 and 48 x 172 = 8 256
# frames, the kernel at 32 x 862 = 27 584, the smallest size at which it was seen to win (x 1.20 at C = 384, x 1.04 at C = 512),
# and at 64 x 862 (x 1.18, x 1.04).
LAYER_TORCH_FASTER = {384: 27584, 512: 27584}
# C -> the number of frames B T below which the channel-split form (csrc/wavenet_split.h) was MEASURED faster than both the torch
# chain and the tiled form (tools/wavenet_bench.py --mode split, profiles/wavenet_split_latency.json): the smallest measured size
# at which it was not the fastest of the three (one past the largest measured size if there is none); no entry where it is not
# the fastest at 1 x 100.  On one MI355X, at C = 384 / 512, it was the fastest at 1 x 100, 1 x 203, 4 x 203 and 1 x 862 (x2.17 /
# x2.21, x2.06 / x2.14, x1.42 / x1.48 and x1.41 / x1.28 over torch for a layer) and lost to torch at 48 x 172 = 8 256 frames
# (x0.78 / x0.90): nothing between 862 and 8 256 frames was measured, and the bound is the measured loss.
SPLIT_BELOW = {384: 8256, 512: 8256}
# dispatch counters (tests and tools read them): layer calls ("hip": on the kernel in either form, "split": those of them that
# took the split form); separate from conformer.CALLS
CALLS = {"hip": 0, "reference": 0, "split": 0}
PACKS = {"count": 0}                                   # weight tables built (a cache hit does not count)
_WS = collections.OrderedDict()                        # (device, stream) -> the buffer the split form's gate passes through
_WS_MAX = 8


def tile(C, H):
    """frames per workgroup (``ddsp_hip_wavenet_layer_tile``); 0 for a (C, H) the kernel does not take"""
    return int(_ffi.lib().ddsp_hip_wavenet_layer_tile(int(C), int(H)))


def split_tile(C, H):
    """frames per workgroup of the split form (``ddsp_hip_wavenet_layer_split_tile``); 0 for a shape the kernels do not take"""
    return int(_ffi.lib().ddsp_hip_wavenet_layer_split_tile(int(C), int(H)))


def split_in_range(B, T):
    """the split form takes ``B ceil(T / 16)`` tiles up to ``SPLIT_MAX_TILES`` (``_modules.split_in_range``)"""
    return _modules.split_in_range(B, T)


def choose_form(C, B, T):
    """where the hook sends a layer call of ``B x T`` frames: ``"split"`` within the split form's range below the measured
    ``SPLIT_BELOW[C]``, else ``"tiled"`` unless ``LAYER_TORCH_FASTER`` gives the size to torch, else None (the torch chain):
    ``_modules.choose_form`` on this module's two tables as they are now"""
    return _modules.choose_form(SPLIT_BELOW, LAYER_TORCH_FASTER, C, B, T)


def _workspace(B, T, C, x):
    """the buffer the split form's gate passes through, for ``x``'s device and the caller's stream there
    (``_modules.stream_workspace``'s rule)"""
    nbytes = int(_ffi.lib().ddsp_hip_wavenet_layer_split_workspace_bytes(B, T, C))
    return stream_workspace(_WS, max(nbytes // 4, 4), x, _WS_MAX)


def release_workspace():
    """drop the cached workspaces of the split form"""
    drop_workspaces(_WS)


def _pack(dims, flat):
    """the host table of ``(wdil, bdil, wc, bc, wo, bo)``, for ``packed_table``"""
    lib = _ffi.lib()
    refusal = "residual_layer: (C, H) = (%d, %d) is outside the kernel's range" % dims
    host = pack_host(int(lib.ddsp_hip_wavenet_layer_pack_bytes(*dims)), refusal, flat, lib.ddsp_hip_wavenet_layer_pack, dims)
    PACKS["count"] += 1
    return host


def _check_weights(weights, C, H):
    if len(weights) != 6:
        raise ValueError("residual_layer: weights must be (wdil, bdil, wc, bc, wo, bo)")
    want = ((2 * C, C, 3), (2 * C,), (2 * C, H, 1), (2 * C,), (2 * C, C, 1), (2 * C,))
    if any(tuple(t.shape) != s for t, s in zip(weights, want)):
        raise ValueError("residual_layer: weights must be [2 C, C, 3], [2 C], [2 C, H, 1], [2 C], [2 C, C, 1], [2 C]")


def _result(name, t, like):
    if t is None:
        return torch.empty_like(like)
    if not t.is_contiguous() or t.shape != like.shape or t.dtype != torch.float32:
        raise ValueError("residual_layer: %s must be a contiguous float32 tensor of x's shape" % name)
    return t


def residual_layer(x, cond, d, weights, out=None, skip=None, accumulate=False, form="tiled", ws=None):
    """One residual layer on the HIP kernel: ``x [B, C, T]``, ``cond [B, H, T]``, ``d [B, C]`` (the layer's projection of the
    step embedding), ``weights = (wdil [2 C, C, 3], bdil [2 C], wc [2 C, H, 1], bc [2 C], wo [2 C, C, 1], bo [2 C])``, all float32.
    Returns ``(x_out, skip)``: ``(x + residual) / sqrt 2`` in ``out`` and the skip half in ``skip`` -- with ``accumulate`` ADDED
    to what ``skip`` holds.  ``out`` must not be ``x`` (a tile reads its neighbours' frames).  ``form``: ``"tiled"``
    (csrc/wavenet_layer.h, one launch) or ``"split"`` (csrc/wavenet_split.h, two launches with a frame tile of 16 for calls of a
    few hundred frames, ``B ceil(T / 16) <= 4096``, ValueError beyond); both give the same bits.  ``ws`` (split form only): a
    float32 buffer of at least ``B T C`` elements for the gate, instead of the cached one of the caller's stream.  No
    synchronisation; once the weight table (and the split form's workspace) exists the only allocations are the results that were
    not given, so a call can be captured in a graph (a capture of the split form without ``ws`` takes a workspace from the graph's
    pool)."""
    _ffi.check_device(x, cond, d, out, skip)
    if x.dtype != torch.float32 or x.dim() != 3 or cond.dtype != torch.float32 or cond.dim() != 3 or d.dtype != torch.float32:
        raise ValueError("residual_layer: x [B, C, T], cond [B, H, T] and d [B, C] must be float32 tensors")
    B, C, T = x.shape
    H = cond.shape[1]
    if (C, H) not in SHAPES:
        raise ValueError("residual_layer: (C, H) = (%d, %d) is outside the kernel's range" % (C, H))
    if cond.shape[0] != B or cond.shape[2] != T or tuple(d.shape) != (B, C):
        raise ValueError("residual_layer: cond must be [B, H, T] and d [B, C]")
    _check_weights(weights, C, H)
    if T < 1:
        raise ValueError("residual_layer: T must be positive")
    if form not in FORMS:
        raise ValueError("residual_layer: form must be 'tiled' or 'split'")
    if form == "split" and not _modules.split_in_range(B, T):
        raise ValueError("residual_layer: the split form takes B ceil(T / 16) <= %d tiles" % SPLIT_MAX_TILES)
    if out is x or skip is x or (out is not None and out is skip):
        raise ValueError("residual_layer: out and skip must be two tensors, neither of them x")
    if accumulate and skip is None:
        raise ValueError("residual_layer: accumulate needs the skip buffer to add to")
    x, cond, d = x.contiguous(), cond.contiguous(), d.contiguous()
    y, s = _result("out", out, x), _result("skip", skip, x)
    if B == 0:
        return y, s
    table = packed_table("wavenet", (C, H), list(weights), x.device, _pack)
    if form == "split":
        if ws is None:
            ws = _workspace(B, T, C, x)
        elif ws.dtype != torch.float32 or not ws.is_contiguous() or ws.device != x.device:
            raise ValueError("residual_layer: ws must be a contiguous float32 tensor on x's device")
        CALLS["hip"] += 1
        CALLS["split"] += 1
        _ffi.check(_ffi.lib().ddsp_hip_wavenet_layer_split(x.data_ptr(), cond.data_ptr(), d.data_ptr(), y.data_ptr(), s.data_ptr(),
                                                           table.data_ptr(), table.numel() * 4, ws.data_ptr(), ws.numel() * 4, B, T,
                                                           C, H, 1 if accumulate else 0, _ffi.stream_of(x)))
        return y, s
    CALLS["hip"] += 1
    _ffi.check(_ffi.lib().ddsp_hip_wavenet_layer(x.data_ptr(), cond.data_ptr(), d.data_ptr(), y.data_ptr(), s.data_ptr(),
                                                 table.data_ptr(), table.numel() * 4, B, T, C, H, 1 if accumulate else 0,
                                                 _ffi.stream_of(x)))
    return y, s


def residual_stack(x, cond, s, layers, form="tiled"):
    """The residual layers of a WaveNet: ``x [B, C, T]``, ``cond [B, H, T]``, ``s [B, C]`` (the step embedding after the mlp),
    ``layers`` a list of ``(weights, (wp [C, C], bp [C]))``.  The projections of all layers are ONE matmul; then one launch per
    layer, x handed over through two buffers (the caller's x is never written), the first layer stores its skip half and the
    others add theirs to it.  ``form`` as in ``residual_layer``, for every layer; the split form uses one workspace for all
    layers (in a graph capture as well).  Returns ``(x after the last layer, the sum of the skips)``."""
    if not layers:
        raise ValueError("residual_stack: no layers")
    if form not in FORMS or (form == "split" and (x.dim() != 3 or not _modules.split_in_range(x.shape[0], x.shape[2]))):
        raise ValueError("residual_stack: form must be 'tiled' or 'split', the latter with B ceil(T / 16) <= %d" % SPLIT_MAX_TILES)
    n, C = len(layers), x.shape[1]
    d = step_biases(s, [p for _, p in layers])                                            # [n, B, C]
    cond = cond.contiguous()
    bufs = (torch.empty_like(x, memory_format=torch.contiguous_format),
            torch.empty_like(x, memory_format=torch.contiguous_format) if n > 1 else None)
    skip = torch.empty_like(bufs[0])
    ws = _workspace(x.shape[0], x.shape[2], C, x) if form == "split" and x.shape[0] and x.shape[2] else None
    src = x
    for i, (weights, _) in enumerate(layers):
        dst = bufs[i % 2]
        residual_layer(src, cond, d[i], weights, out=dst, skip=skip, accumulate=i > 0, form=form, ws=ws)
        src = dst
    return src, skip


# ---- the reference's modules --------------------------------------------------------------------------------------------------

def _conv(c, cin, cout, k, pad):
    return (isinstance(c, torch.nn.Conv1d) and plain_with_bias(c) and c.in_channels == cin and c.out_channels == cout
            and c.kernel_size == (k,) and c.stride == (1,) and c.dilation == (1,) and c.groups == 1 and pad_of(c) == (pad,)
            and c.padding_mode == "zeros")


def _layer_spec(block):
    """``(weights, (wp, bp))`` of a module with the residual block's four submodules in the kernel's shapes, or None"""
    dil, proj = getattr(block, "dilated_conv", None), getattr(block, "diffusion_projection", None)
    cp, op = getattr(block, "conditioner_projection", None), getattr(block, "output_projection", None)
    if not isinstance(block, torch.nn.Module) or block._forward_pre_hooks or block._forward_hooks:
        return None
    if not isinstance(dil, torch.nn.Conv1d) or not isinstance(cp, torch.nn.Conv1d):
        return None
    C, H = dil.in_channels, cp.in_channels
    if getattr(block, "residual_channels", C) != C:
        return None
    if not _conv(dil, C, 2 * C, 3, 1) or not _conv(cp, H, 2 * C, 1, 0) or not _conv(op, C, 2 * C, 1, 0):
        return None
    if not isinstance(proj, torch.nn.Linear) or not plain_with_bias(proj) or proj.in_features != C or proj.out_features != C:
        return None
    return (dil.weight, dil.bias, cp.weight, cp.bias, op.weight, op.bias), (proj.weight, proj.bias)


def layer_eligible(block, x, cond, s):
    """the ``(weights, (wp, bp))`` to run ``block`` on ``(x, cond, s)`` with the HIP kernel (in the form ``choose_form`` names for
    the size), or None: the block's own forward"""
    if not on_device(x, 3) or not on_device(cond, 3) or not on_device(s, 2) or x.shape[2] < 1:
        return None
    if autocast_on(x):
        return None
    spec = _layer_spec(block)
    if spec is None:
        return None
    weights, proj = spec
    C, H = weights[0].shape[1], weights[2].shape[1]
    B, T = x.shape[0], x.shape[2]
    if (C, H) not in SHAPES or x.shape[1] != C or tuple(cond.shape) != (B, H, T) or tuple(s.shape) != (B, C):
        return None
    flat = list(weights) + list(proj)
    if any(t.device != x.device for t in flat + [cond, s]) or needs_grad([x, cond, s] + flat):
        return None
    if choose_form(C, B, T) is None:
        return None
    return spec


def _reference_layer_forward(block, x, conditioner, diffusion_step):
    CALLS["reference"] += 1
    return run_reference(block, getattr(block, "reference_forward", None), x, conditioner, diffusion_step)


def layer_forward(block, x, conditioner, diffusion_step):
    """the dispatcher bound as ``ResidualBlock.forward``"""
    spec = layer_eligible(block, x, conditioner, diffusion_step)
    if spec is None:
        return _reference_layer_forward(block, x, conditioner, diffusion_step)
    weights, (wp, bp) = spec
    form = choose_form(x.shape[1], x.shape[0], x.shape[2])
    return residual_layer(x, conditioner, torch.addmm(bp, diffusion_step, wp.t()), weights, form=form)


def net_forward(wavenet, spec, diffusion_step, cond):
    """the dispatcher bound as ``WaveNet.forward``: the module's own submodules around the residual layers; the layers as
    ``residual_stack`` (one form for all layers: ``choose_form``) when every one of them is eligible, each through its own
    forward otherwise"""
    x = torch.relu(wavenet.input_projection(spec.squeeze(1)))
    s = wavenet.mlp(wavenet.diffusion_embedding(diffusion_step))
    blocks = list(wavenet.residual_layers)
    specs = [layer_eligible(blk, x, cond, s) for blk in blocks] if blocks else [None]
    if all(sp is not None for sp in specs):
        _, total = residual_stack(x, cond, s, specs, choose_form(x.shape[1], x.shape[0], x.shape[2]))
    else:
        skips = []
        for blk in blocks:
            x, skip = blk(x, cond, s)
            skips.append(skip)
        total = torch.sum(torch.stack(skips), dim=0)
    x = total / math.sqrt(len(blocks))
    x = torch.relu(wavenet.skip_projection(x))
    return wavenet.output_projection(x)[:, None, :, :]


_REFERENCE_MODULE = "diffusion.wavenet"
_CLASSES = (("ResidualBlock", lambda self, x, conditioner, diffusion_step: layer_forward(self, x, conditioner, diffusion_step)),
            ("WaveNet", lambda self, spec, diffusion_step, cond: net_forward(self, spec, diffusion_step, cond)))


def patch_reference_wavenet():
    """Route ``ResidualBlock.forward`` and ``WaveNet.forward`` of ``diffusion.wavenet`` through the dispatchers above.
    Idempotent; returns the module, or None when it does not import.  ``vocoder.patch_reference()`` does not call it: the hook
    is opt-in."""
    return (patch_forwards([_REFERENCE_MODULE], _CLASSES) or [None])[0]


def unpatch_reference_wavenet():
    """Undo ``patch_reference_wavenet()``."""
    unpatch_forwards([_REFERENCE_MODULE], [name for name, _ in _CLASSES])
