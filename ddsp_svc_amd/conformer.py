"""The conformer conv module of the control network (``ConformerConvModule`` of ``diffusion.model_conformer_naive``, the same
text in ``reflow``, the same mathematics in ``ddsp.pcmer``) on HIP: csrc/conformer_conv.h, one launch per module call, both
pointwise convolutions as f32 MFMA GEMMs, the GLU, the 31-tap depthwise convolution and the SiLU between them on the CU.

  tile                          output frames per workgroup (``ddsp_hip_conformer_conv_tile``)
  conv_module                   the functional form: ``x [B, L, D]``, ``(w1, b1, wd, bd, w2, b2)``, an optional LayerNorm in front
  encoder                       ``x = x + net_i(x)`` over a list of layers, one call each, ping-pong between two buffers
  choose_form                   ``"split"``, ``"tiled"`` or None (torch) for a size, from the two measured tables
  conv_forward / layer_forward  the dispatchers bound as ``ConformerConvModule.forward`` / ``CFNEncoderLayer.forward``
  encoder_forward               the dispatcher bound as ``ConformerNaiveEncoder.forward``: where the hook takes the split form
  patch_reference_conformer     rebinds those three in whichever reference modules import; opt-in (``patch_reference`` leaves it)
  unpatch_reference_conformer
  release_workspace             drop the cached workspaces of the split form

Dispatch (``conv_eligible``) is decided from a module's structure, not its class: a ``net`` Sequential of ``[LayerNorm(D) |
Identity, Transpose, Conv1d(D, 4 D, 1), GLU(dim=1), depthwise Conv1d(2 D, 2 D, 31, padding 15, groups 2 D) or pcmer's pad-then-conv
wrapper, SiLU | Swish, Conv1d(2 D, D, 1), Transpose, Dropout]`` with D = 256, plain float32 parameters without hooks, the
dropout inactive, a float32 ``[B, L, 256]`` tensor on the GPU, no gradient needed and autocast off.  Everything else -- D = 512,
other tap counts, weight norm, training, CPU tensors, parameters that are inference tensors -- runs the module's own ``net``.
``CONV_TORCH_FASTER`` maps D to the number of frames B L below which the same-GPU torch chain was measured faster
(tools/conformer_bench.py).

The module has a second form, csrc/conformer_split.h (``form="split"``): the same sums in the same order, hence the same bits, with
a frame tile of 16 and the channels split over workgroups, three launches and a workspace, for calls of a few hundred frames
(``B ceil(L / 16) <= 4096``).  ``CONV_SPLIT_BELOW`` maps D to the number of frames below which it was measured the fastest of the
three sides.  The hook takes it in ONE place, ``encoder_forward``: a conv-only ``ConformerNaiveEncoder`` (the decoder of
``Unit2Control(use_naive_v2=True)``) whose size ``choose_form`` gives to the split form runs all its layers there under one
workspace.  A bare module call, a single ``CFNEncoderLayer`` and the conv modules inside ``PCmer``'s layers keep the two-way
routing above: at real-time sizes they stay on torch.
"""
import collections

import torch

from . import _ffi, _modules
from ._modules import (FORMS, SPLIT_MAX_TILES, autocast_on, drop_workspaces, needs_grad, on_device, pack_host, packed_table,
                       pad_of, plain_with_bias, pointwise, stream_workspace, torch_faster, tracked)
from ._patching import patch_forwards, run_reference, unpatch_forwards

DIMS = (256,)
TAPS = 31
# D -> the number of frames B L below which the torch op chain was measured faster on the same GPU (None: at every size).
# tools/conformer_bench.py on one MI355X (profiles/conformer_throughput.json, conformer_latency.json): torch is faster at
# 1 x 100, 1 x 203 and 48 x 172 = 8 256 frames, the kernel at 32 x 862 = 27 584, the smallest size at which it was seen to win.
CONV_TORCH_FASTER = {256: 27584}
# D -> the number of frames B L below which the channel-split form (csrc/conformer_split.h) was MEASURED faster than both the
# torch chain and the tiled form (tools/conformer_bench.py --mode split, profiles/conformer_split_latency.json): the smallest
# measured size at which it was not the fastest of the three; no entry where it is not the fastest at 1 x 100.  On one MI355X it
# was the fastest at all five measured sizes -- 1 x 100, 1 x 203, 4 x 203, 1 x 862 and 48 x 172 = 8 256 frames (x2.55, x2.47, x1.78,
# x1.82 and x1.37 over torch, the tiled form behind both) --, so the bound is one past the largest of them: nothing above it was
# measured.
CONV_SPLIT_BELOW = {256: 8257}
# dispatch counters (tests and tools read them): module calls ("hip": on the kernels in either form, "split": those of them that
# took the split form); separate from nsf_generator.CALLS
CALLS = {"hip": 0, "reference": 0, "split": 0}
PACKS = {"count": 0}                                   # weight tables built (a cache hit does not count)
_WS = collections.OrderedDict()                        # (device, stream) -> the buffer the split form's g and h pass through
_WS_MAX = 16


def tile(D):
    """output frames per workgroup (``ddsp_hip_conformer_conv_tile``); 0 for a D the kernel does not take"""
    return int(_ffi.lib().ddsp_hip_conformer_conv_tile(int(D)))


def split_tile(D):
    """frames per workgroup of the split form; 0 for a D the kernels do not take"""
    return int(_ffi.lib().ddsp_hip_conformer_conv_split_tile(int(D)))


def split_in_range(B, L):
    """the split form takes ``B ceil(L / 16)`` tiles up to ``SPLIT_MAX_TILES`` (``_modules.split_in_range``)"""
    return _modules.split_in_range(B, L)


def choose_form(D, B, L):
    """where ``encoder_forward`` sends an encoder call of ``B x L`` frames: ``"split"`` within the split form's range below the
    measured ``CONV_SPLIT_BELOW[D]``, else ``"tiled"`` unless ``CONV_TORCH_FASTER`` gives the size to torch, else None (the torch
    chain): ``_modules.choose_form`` on this module's two tables as they are now"""
    return _modules.choose_form(CONV_SPLIT_BELOW, CONV_TORCH_FASTER, D, B, L)


def _workspace(B, L, D, x):
    """the buffer the split form's intermediates (the GLU's output and the stencil's) pass through, for ``x``'s device and the
    caller's stream there (``_modules.stream_workspace``'s rule)"""
    size = int(_ffi.lib().ddsp_hip_conformer_conv_split_workspace_bytes(B, L, D))
    return stream_workspace(_WS, max(size // 4, 4), x, _WS_MAX)


def release_workspace():
    """drop the cached hand-over buffers of every device and stream"""
    drop_workspaces(_WS)


def _pack(dims, flat):
    """the host table of ``(w1, b1, wd, bd, w2, b2)`` and, with ``dims = (D, True)``, ``(gamma, beta)``, for ``packed_table``"""
    (D, normed), lib = dims, _ffi.lib()
    refusal = "conv_module: D = %d is outside the kernel's range" % D
    host = pack_host(int(lib.ddsp_hip_conformer_conv_pack_bytes(D, int(normed))), refusal, flat, lib.ddsp_hip_conformer_conv_pack,
                     (D,) if normed else (None, None, D))                    # no LayerNorm: no gamma and beta to pack
    PACKS["count"] += 1
    return host


def _check_weights(weights, norm, D):
    if len(weights) != 6:
        raise ValueError("conv_module: weights must be (w1, b1, wd, bd, w2, b2)")
    w1, b1, wd, bd, w2, b2 = weights
    want = ((4 * D, D, 1), (4 * D,), (2 * D, 1, TAPS), (2 * D,), (D, 2 * D, 1), (D,))
    if any(tuple(t.shape) != s for t, s in zip(weights, want)):
        raise ValueError("conv_module: weights must be [4 D, D, 1], [4 D], [2 D, 1, 31], [2 D], [D, 2 D, 1], [D]")
    if norm is not None and (len(norm) != 2 or any(tuple(t.shape) != (D,) for t in norm)):
        raise ValueError("conv_module: norm must be (gamma [D], beta [D])")


def conv_module(x, weights, norm=None, eps=1e-5, add_input=False, out=None, form="tiled", ws=None):
    """``net(x)`` of a conformer conv module on the HIP kernels (``x + net(x)`` with ``add_input``): ``x [B, L, D]`` float32,
    ``weights = (w1 [4 D, D, 1], b1 [4 D], wd [2 D, 1, 31], bd [2 D], w2 [D, 2 D, 1], b2 [D])``, ``norm = (gamma [D], beta [D])`` of
    the LayerNorm in front or None.  ``out`` must not be ``x``: a tile reads its neighbours' frames.  ``form``: ``"tiled"``
    (csrc/conformer_conv.h, one launch) or ``"split"`` (csrc/conformer_split.h, three launches with a frame tile of 16 for calls of a
    few hundred frames, ``B ceil(L / 16) <= 4096``, ValueError beyond); both read one packed table and give the same bits.  ``ws``
    (split form only): a float32 buffer of at least ``4 B L D`` elements for the intermediates, instead of the cached one of the
    caller's stream.  No synchronisation; once the weight table (and the workspace) exists the only allocation is the result
    (when ``out`` is None), so a call can be captured in a graph (a split capture without ``ws`` takes a workspace from the
    graph's pool)."""
    _ffi.check_device(x, out)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError("conv_module: x must be a float32 [B, L, D] tensor")
    B, L, D = x.shape
    if D not in DIMS:
        raise ValueError("conv_module: D = %d is outside the kernel's range" % D)
    _check_weights(weights, norm, D)
    if L < 1:
        raise ValueError("conv_module: L must be positive")
    if form not in FORMS:
        raise ValueError("conv_module: form must be 'tiled' or 'split'")
    if form == "split" and not _modules.split_in_range(B, L):
        raise ValueError("conv_module: the split form takes B ceil(L / 16) <= %d tiles" % SPLIT_MAX_TILES)
    if out is x:
        raise ValueError("conv_module: out must not be x")
    x = x.contiguous()
    y = torch.empty_like(x) if out is None else out
    if not y.is_contiguous() or y.shape != x.shape or y.dtype != torch.float32:
        raise ValueError("conv_module: out must be a contiguous float32 tensor of x's shape")
    if B == 0:
        return y
    flat = list(weights) + (list(norm) if norm is not None else [])
    table = packed_table("conformer", (D, norm is not None), flat, x.device, _pack)
    tail = (B, L, D, 0 if norm is None else 1, float(eps), 1 if add_input else 0, _ffi.stream_of(x))
    if form == "split":
        if ws is None:
            ws = _workspace(B, L, D, x)
        elif (not isinstance(ws, torch.Tensor) or ws.dtype != torch.float32 or not ws.is_contiguous()
              or ws.device != x.device):
            raise ValueError("conv_module: ws must be a contiguous float32 tensor on x's device")
        CALLS["hip"] += 1
        CALLS["split"] += 1
        _ffi.check(_ffi.lib().ddsp_hip_conformer_conv_split(x.data_ptr(), y.data_ptr(), table.data_ptr(), table.numel() * 4,
                                                            ws.data_ptr(), ws.numel() * 4, *tail))
        return y
    CALLS["hip"] += 1
    _ffi.check(_ffi.lib().ddsp_hip_conformer_conv(x.data_ptr(), y.data_ptr(), table.data_ptr(), table.numel() * 4, *tail))
    return y


def encoder(x, layers, out=None, form="tiled"):
    """``x = x + net_i(x)`` over ``layers``, a list of ``(weights, norm, eps)``: one call per layer, the layers hand over through
    two buffers (the result and one more), ``x`` itself is never written.  ``form`` as in ``conv_module``, for every layer; the
    split form's layers share one workspace (in a graph capture as well).  Returns the result (``out`` when given)."""
    if not layers:
        raise ValueError("encoder: no layers")
    if out is x:
        raise ValueError("encoder: out must not be x")
    if form not in FORMS:
        raise ValueError("encoder: form must be 'tiled' or 'split'")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] < 1:
        raise ValueError("encoder: x must be a float32 [B, L, D] tensor, L positive")
    B, L, D = x.shape
    if form == "split" and not _modules.split_in_range(B, L):
        raise ValueError("encoder: the split form takes B ceil(L / 16) <= %d tiles" % SPLIT_MAX_TILES)
    _ffi.check_device(x, out)
    ws = _workspace(B, L, D, x) if form == "split" and B else None
    n = len(layers)
    a = torch.empty_like(x, memory_format=torch.contiguous_format) if out is None else out
    b = torch.empty_like(a) if n > 1 else None
    src = x
    for i, (weights, norm, eps) in enumerate(layers):
        dst = a if (n - 1 - i) % 2 == 0 else b         # the last layer writes the result
        conv_module(src, weights, norm=norm, eps=eps, add_input=True, out=dst, form=form, ws=ws)
        src = dst
    return a


# ---- the reference's modules --------------------------------------------------------------------------------------------------

def _depthwise(m, C):
    """the depthwise Conv1d of either form: ``Conv1d(C, C, 31, padding=15, groups=C)``, or a wrapper that pads by (15, 15) and
    then runs an unpadded grouped ``conv``"""
    if isinstance(m, torch.nn.Conv1d):
        conv, pad = m, pad_of(m)
        pad = (pad[0], pad[0])
        if m.padding_mode != "zeros":
            return None
    else:
        conv, pad = getattr(m, "conv", None), getattr(m, "padding", None)
        if not isinstance(conv, torch.nn.Conv1d) or not isinstance(pad, (tuple, list)) or pad_of(conv) != (0,):
            return None
        if not isinstance(m, torch.nn.Module) or m._forward_pre_hooks or m._forward_hooks:
            return None
        pad = tuple(pad)
    if (pad != (TAPS // 2, TAPS // 2) or not plain_with_bias(conv) or conv.in_channels != C or conv.out_channels != C
            or conv.groups != C or conv.kernel_size != (TAPS,) or conv.stride != (1,) or conv.dilation != (1,)):
        return None
    return conv


def _is_transpose(m):
    return type(m).__name__ == "Transpose" and tuple(getattr(m, "dims", ())) == (1, 2)


def _conv_spec(module):
    """``(weights, norm, eps, dropout)`` of a module whose ``net`` is the conformer conv chain, or None"""
    net = getattr(module, "net", None)
    if not isinstance(net, torch.nn.Sequential) or len(net) != 9:
        return None
    if module._forward_pre_hooks or module._forward_hooks or net._forward_pre_hooks or net._forward_hooks:
        return None
    ln, t1, c1, glu, dw, act, c2, t2, drop = net
    if not isinstance(c1, torch.nn.Conv1d):
        return None
    D = c1.in_channels
    if isinstance(ln, torch.nn.LayerNorm):
        if (tuple(ln.normalized_shape) != (D,) or not ln.elementwise_affine or ln.weight is None or ln.bias is None
                or ln.weight.dtype != torch.float32 or ln._forward_pre_hooks or ln._forward_hooks
                or not tracked(ln.weight, ln.bias)):
            return None
        norm, eps = (ln.weight, ln.bias), ln.eps
    elif isinstance(ln, torch.nn.Identity):
        norm, eps = None, 1e-5
    else:
        return None
    if not _is_transpose(t1) or not _is_transpose(t2) or not isinstance(drop, torch.nn.Dropout):
        return None
    if not (isinstance(glu, torch.nn.GLU) or type(glu).__name__ == "GLU") or getattr(glu, "dim", None) != 1:
        return None
    if not (isinstance(act, torch.nn.SiLU) or type(act).__name__ == "Swish"):
        return None
    if any(m._forward_pre_hooks or m._forward_hooks for m in (t1, glu, act, t2, drop)):
        return None
    if not pointwise(c1, D, 4 * D) or not pointwise(c2, 2 * D, D):
        return None
    conv = _depthwise(dw, 2 * D)
    if conv is None:
        return None
    return (c1.weight, c1.bias, conv.weight, conv.bias, c2.weight, c2.bias), norm, eps, drop


def _tensor_ok(x):
    """the clauses of ``conv_eligible`` about ``x`` alone: float32 ``[B, L >= 1, D]`` on the device, autocast off"""
    return on_device(x, 3) and x.shape[1] >= 1 and not autocast_on(x)


def _structural(module, x):
    """the structural part of ``conv_eligible``, without the measured table: the ``(weights, norm, eps)`` of a ``module`` in the
    kernels' form (``_conv_spec``, D in range and ``x``'s, the dropout inactive, the parameters on ``x``'s device, no gradient
    needed), or None.  ``x`` has passed ``_tensor_ok``."""
    spec = _conv_spec(module)
    if spec is None:
        return None
    weights, norm, eps, drop = spec
    D = weights[0].shape[1]
    if D not in DIMS or x.shape[-1] != D:
        return None
    if drop.p != 0 and drop.training:
        return None
    flat = list(weights) + (list(norm) if norm is not None else [])
    if any(t.device != x.device for t in flat) or needs_grad([x] + flat):
        return None
    return weights, norm, eps


def conv_eligible(module, x):
    """the ``(weights, norm, eps)`` to run ``module`` on ``x`` with the HIP kernel, or None: the module's own ``net``"""
    if not _tensor_ok(x):
        return None
    spec = _structural(module, x)
    if spec is None or torch_faster(CONV_TORCH_FASTER, x.shape[-1], x.shape[0] * x.shape[1]):
        return None
    return spec


def _reference_conv_forward(module, x):
    CALLS["reference"] += 1
    return run_reference(module, getattr(module, "net", None), x)


def conv_forward(module, x):
    """the dispatcher bound as ``ConformerConvModule.forward``"""
    spec = conv_eligible(module, x)
    if spec is None:
        return _reference_conv_forward(module, x)
    return conv_module(x, spec[0], norm=spec[1], eps=spec[2])


def layer_forward(layer, x, mask=None):
    """the dispatcher bound as ``CFNEncoderLayer.forward``: a conv-only layer whose conv module is eligible is one launch with the
    residual add inside; otherwise the reference's two lines (the conv module then dispatches for itself)"""
    if layer.attn is None:
        spec = conv_eligible(layer.conformer, x)
        if spec is not None:
            return conv_module(x, spec[0], norm=spec[1], eps=spec[2], add_input=True)
    else:
        x = x + (layer.attn(layer.norm(x), mask=mask))
    x = x + (layer.conformer(x))
    return x


def _hooked(module):
    return bool(module._forward_pre_hooks or module._forward_hooks)


def _split_encoder_specs(enc, x):
    """the ``(weights, norm, eps)`` of every layer when ``enc`` on ``x`` is the split form's: a non-empty ``encoder_layers`` of
    conv-only layers, none of them or of their conv modules carrying a forward hook or pre-hook (the direct call would skip it),
    every conv module structurally eligible, the clauses of ``conv_eligible`` on ``x``, and a size ``choose_form`` gives to the
    split form; None otherwise"""
    layers = getattr(enc, "encoder_layers", None)
    if layers is None or len(layers) == 0 or not _tensor_ok(x):
        return None
    if choose_form(x.shape[2], x.shape[0], x.shape[1]) != "split":
        return None
    specs = []
    for layer in layers:
        conv = getattr(layer, "conformer", None)
        if (not isinstance(layer, torch.nn.Module) or getattr(layer, "attn", True) is not None
                or not isinstance(conv, torch.nn.Module) or _hooked(layer) or _hooked(conv)):
            return None
        spec = _structural(conv, x)
        if spec is None:
            return None
        specs.append(spec)
    return specs


def encoder_forward(enc, x, mask=None):
    """the dispatcher bound as ``ConformerNaiveEncoder.forward``: a conv-only encoder at a size ``choose_form`` gives to the split
    form runs ``encoder(..., form="split")``, all layers under one workspace; everything else is the reference's own loop, whose
    layers then dispatch one by one as ``layer_forward`` decides (``mask`` only reaches attention layers)"""
    specs = _split_encoder_specs(enc, x) if isinstance(x, torch.Tensor) else None
    if specs is not None:
        return encoder(x, specs, form="split")
    for layer in enc.encoder_layers:
        x = layer(x, mask)
    return x


_REFERENCE_MODULES = ("diffusion.model_conformer_naive", "reflow.model_conformer_naive", "ddsp.pcmer")


_CLASSES = (("ConformerConvModule", lambda self, x: conv_forward(self, x)),
            ("CFNEncoderLayer", lambda self, x, mask=None: layer_forward(self, x, mask)),
            ("ConformerNaiveEncoder", lambda self, x, mask=None: encoder_forward(self, x, mask)))


def patch_reference_conformer():
    """Route ``ConformerConvModule.forward``, ``CFNEncoderLayer.forward`` and ``ConformerNaiveEncoder.forward`` of whichever of
    the reference's modules import (``diffusion.model_conformer_naive``, ``reflow.model_conformer_naive``, ``ddsp.pcmer``, which
    needs local_attention and has no ``ConformerNaiveEncoder``) through the dispatchers above.  Idempotent; returns the list of
    modules patched.  ``vocoder.patch_reference()`` does not call it: the hook is opt-in."""
    return patch_forwards(_REFERENCE_MODULES, _CLASSES)


def unpatch_reference_conformer():
    """Undo ``patch_reference_conformer()``."""
    unpatch_forwards(_REFERENCE_MODULES, [name for name, _ in _CLASSES])
