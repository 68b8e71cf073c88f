"""The conformer conv module of the control network (``ConformerConvModule`` of ``diffusion.model_conformer_naive``, the same
text in ``reflow``, the same mathematics in ``ddsp.pcmer``) on HIP: csrc/conformer_conv.h, one launch per module call, both
pointwise convolutions as f32 MFMA GEMMs, the GLU, the 31-tap depthwise convolution and the SiLU between them on the CU.

  tile                          output frames per workgroup (``ddsp_hip_conformer_conv_tile``)
  conv_module                   the functional form: ``x [B, L, D]``, ``(w1, b1, wd, bd, w2, b2)``, an optional LayerNorm in front
  encoder                       ``x = x + net_i(x)`` over a list of layers, one launch each, ping-pong between two buffers
  conv_forward / layer_forward  the dispatchers bound as ``ConformerConvModule.forward`` / ``CFNEncoderLayer.forward``
  patch_reference_conformer     rebinds those two in whichever reference modules import; opt-in (``patch_reference`` leaves it)
  unpatch_reference_conformer

Dispatch (``conv_eligible``) is decided from a module's structure, not its class: a ``net`` Sequential of ``[LayerNorm(D) |
Identity, Transpose, Conv1d(D, 4 D, 1), GLU(dim=1), depthwise Conv1d(2 D, 2 D, 31, padding 15, groups 2 D) or pcmer's pad-then-conv
wrapper, SiLU | Swish, Conv1d(2 D, D, 1), Transpose, Dropout]`` with D = 256, plain float32 parameters without hooks, the
dropout inactive, a float32 ``[B, L, 256]`` tensor on the GPU, no gradient needed and autocast off.  Everything else -- D = 512,
other tap counts, weight norm, training, CPU tensors, parameters that are inference tensors -- runs the module's own ``net``.
``CONV_TORCH_FASTER`` maps D to the number of frames B L below which the same-GPU torch chain was measured faster
(tools/conformer_bench.py).
"""
import torch

from . import _ffi
from ._modules import (autocast_on, needs_grad, on_device, pack_host, packed_table, pad_of, plain_with_bias, pointwise,
                       torch_faster, tracked)
from ._patching import patch_forwards, run_reference, unpatch_forwards

DIMS = (256,)
TAPS = 31
# D -> the number of frames B L below which the torch op chain was measured faster on the same GPU (None: at every size).
# tools/conformer_bench.py on one MI355X (profiles/conformer_throughput.json, conformer_latency.json): torch is faster at
# 1 x 100, 1 x 203 and 48 x 172 = 8 256 frames, the kernel at 32 x 862 = 27 584, the smallest size at which it was seen to win.
CONV_TORCH_FASTER = {256: 27584}
# dispatch counters (tests and tools read them): module calls; separate from nsf_generator.CALLS
CALLS = {"hip": 0, "reference": 0}
PACKS = {"count": 0}                                   # weight tables built (a cache hit does not count)


def tile(D):
    """output frames per workgroup (``ddsp_hip_conformer_conv_tile``); 0 for a D the kernel does not take"""
    return int(_ffi.lib().ddsp_hip_conformer_conv_tile(int(D)))


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


def conv_module(x, weights, norm=None, eps=1e-5, add_input=False, out=None):
    """``net(x)`` of a conformer conv module on the HIP kernel (``x + net(x)`` with ``add_input``): ``x [B, L, D]`` float32,
    ``weights = (w1 [4 D, D, 1], b1 [4 D], wd [2 D, 1, 31], bd [2 D], w2 [D, 2 D, 1], b2 [D])``, ``norm = (gamma [D], beta [D])`` of
    the LayerNorm in front or None.  ``out`` must not be ``x``: a tile reads its neighbours' frames.  No synchronisation; once the
    weight table exists the only allocation is the result (when ``out`` is None), so a call can be captured in a graph."""
    _ffi.check_device(x, out)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError("conv_module: x must be a float32 [B, L, D] tensor")
    B, L, D = x.shape
    if D not in DIMS:
        raise ValueError("conv_module: D = %d is outside the kernel's range" % D)
    _check_weights(weights, norm, D)
    if L < 1:
        raise ValueError("conv_module: L must be positive")
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
    CALLS["hip"] += 1
    _ffi.check(_ffi.lib().ddsp_hip_conformer_conv(x.data_ptr(), y.data_ptr(), table.data_ptr(), table.numel() * 4, B, L, D,
                                                  0 if norm is None else 1, float(eps), 1 if add_input else 0,
                                                  _ffi.stream_of(x)))
    return y


def encoder(x, layers, out=None):
    """``x = x + net_i(x)`` over ``layers``, a list of ``(weights, norm, eps)``: one launch per layer, the layers hand over through
    two buffers (the result and one more), ``x`` itself is never written.  Returns the result (``out`` when given)."""
    if not layers:
        raise ValueError("encoder: no layers")
    if out is x:
        raise ValueError("encoder: out must not be x")
    n = len(layers)
    a = torch.empty_like(x, memory_format=torch.contiguous_format) if out is None else out
    b = torch.empty_like(a) if n > 1 else None
    src = x
    for i, (weights, norm, eps) in enumerate(layers):
        dst = a if (n - 1 - i) % 2 == 0 else b         # the last layer writes the result
        conv_module(src, weights, norm=norm, eps=eps, add_input=True, out=dst)
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


def conv_eligible(module, x):
    """the ``(weights, norm, eps)`` to run ``module`` on ``x`` with the HIP kernel, or None: the module's own ``net``"""
    if not on_device(x, 3) or x.shape[1] < 1 or autocast_on(x):
        return None
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
    if torch_faster(CONV_TORCH_FASTER, D, x.shape[0] * x.shape[1]):
        return None
    return weights, norm, eps


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


_REFERENCE_MODULES = ("diffusion.model_conformer_naive", "reflow.model_conformer_naive", "ddsp.pcmer")


_CLASSES = (("ConformerConvModule", lambda self, x: conv_forward(self, x)),
            ("CFNEncoderLayer", lambda self, x, mask=None: layer_forward(self, x, mask)))


def patch_reference_conformer():
    """Route ``ConformerConvModule.forward`` and ``CFNEncoderLayer.forward`` of whichever of the reference's modules import
    (``diffusion.model_conformer_naive``, ``reflow.model_conformer_naive``, ``ddsp.pcmer``, which needs local_attention) through
    the dispatchers above.  Idempotent; returns the list of modules patched.  ``vocoder.patch_reference()`` does not call it:
    the hook is opt-in."""
    return patch_forwards(_REFERENCE_MODULES, _CLASSES)


def unpatch_reference_conformer():
    """Undo ``patch_reference_conformer()``."""
    unpatch_forwards(_REFERENCE_MODULES, [name for name, _ in _CLASSES])
