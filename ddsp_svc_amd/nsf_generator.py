"""The residual blocks of the NSF-HiFiGAN generator (``nsf_hifigan.models.ResBlock1`` and the sum over the blocks of an
upsampling stage in ``Generator.forward``) on HIP: csrc/resblock.h, one launch per conv pair, both convolutions of a pair as
f32 MFMA GEMMs with the intermediate in LDS, and the ``xs / num_kernels`` sum folded into the last launch of each block.

  resblock1                  the functional form: ``x [B, C, T]``, one ``(w1, b1, w2, b2)`` per pair, the dilations
  mrf_stage                  ``sum(block_j(x)) / len(blocks)`` of one stage, accumulated and divided in the kernels' epilogue
  upsample_stage             the seam in front of a stage (csrc/generator_tail.h): ``ConvTranspose1d(lrelu(x)) + noise_conv(source)``
                             in one launch, the transposed convolution as polyphase f32 MFMA GEMMs
  output_head                ``tanh(conv_post(lrelu(x)))``, one vector kernel
  generator_forward          ``Generator.forward`` of any module with the reference generator's attributes, stage by stage
  patch_reference_generator  rebinds ``ResBlock1.forward`` and ``Generator.forward`` of an importable reference checkout
  unpatch_reference_generator
  release_workspace, clear_packed   drop the cached hand-over buffers / the cached weight tables (``_modules``)

Dispatch (``hip_eligible``): a float32 tensor on the GPU, no gradient needed, autocast off, C in {16, 32, 64}, k in {3, 7, 11}, dilations the
kernel's LDS image holds, and plain ``Conv1d`` weights -- every conv of the block has had ``remove_weight_norm`` applied (the
weight-norm hook recomputes ``weight`` in a forward pre-hook, which a call that bypasses ``Conv1d.forward`` would never run).
Everything else -- 128 / 256 channels, ``ResBlock2``, training, CPU tensors -- takes the reference's own forward unchanged.
The 128- and 256-channel blocks have a kernel too, the wide form (csrc/resblock_wide.h: one convolution per launch, the input
channels in chunks of 64): ``resblock1`` and ``mrf_stage`` always take them, the hooks only while ``ROUTE_WIDE`` is set
(``patch_reference_generator(wide=True)``, or the flag itself for a stand-in), under the same conditions otherwise.
``TORCH_FASTER`` lists the (C, k) the measurements on one MI355X (tools/resblock_bench.py) found faster as the
torch op chain: those are routed to it as well.

The seam and the head follow the same rules (``seam_eligible``, ``head_eligible``): Cout in {16, 32, 64} from 2 Cout channels,
``ConvTranspose1d(2 Cout, Cout, 2 u, u, padding u / 2)`` with u in {2, 4, 8}, the noise conv ``Conv1d(1, Cout, 2 s, s, padding s // 2)``
with s in {2, 4} or ``Conv1d(1, Cout, 1)``, a source of s u Tin samples; ``Conv1d(C, 1, 7, padding 3)`` for the head.  The 512 -> 256
and 256 -> 128 seams, weight-normed modules and calls that need a gradient run the torch line.  ``SEAM_TORCH_FASTER`` and
``HEAD_TORCH_FASTER`` play ``TORCH_FASTER``'s part (tools/generator_tail_bench.py).
"""
import collections
import ctypes

import torch
import torch.nn.functional as F

from . import _ffi
from ._modules import (autocast_on, clear_packed, drop_workspaces, needs_grad, on_device, packed_table, pad_of,  # noqa: F401
                       plain, stream_workspace, torch_faster)
from ._patching import park, run_reference, unpark

CHANNELS = (16, 32, 64)
WIDE_CHANNELS = (128, 256)                             # the wide form (csrc/resblock_wide.h): one convolution per launch
ROUTE_WIDE = False                                     # the hooks send 128- / 256-channel blocks to it: patch_reference_generator(wide=True)
KERNEL_SIZES = (3, 7, 11)
LRELU_SLOPE = 0.1
# (C, k) -> the number of columns T below which the same-GPU torch chain was measured faster (None: at every T)
# The wide form's entries are profiles/resblock_wide_{latency,throughput}.json's ``torch_faster`` lists (one MI355X, B = 1 x 203
# frames and B = 32 x 861 frames): torch won at both sizes everywhere but at (128, 3), where the kernel won at T = 64 x 861.
TORCH_FASTER = {(256, 3): None, (256, 7): None, (256, 11): None, (128, 3): 64 * 861, (128, 7): None, (128, 11): None}
UPSAMPLE_RATES = (2, 4, 8)
NOISE_STRIDES = (1, 2, 4)
HEAD_SLOPE = 0.01                                      # F.leaky_relu's default, models.py:260
HEAD_TAPS = 7
# (Cout, u) -> the number of input columns Tin below which the torch chain was measured faster (None: at every Tin); C -> T
SEAM_TORCH_FASTER = {}
HEAD_TORCH_FASTER = {}

_WS = collections.OrderedDict()                        # (device, stream) -> the hand-over buffer between pairs
_WS_MAX = 16
# dispatch counters (tests and tools read them): "hip" / "reference" count residual blocks, the others seams and heads
CALLS = {"hip": 0, "reference": 0, "seam_hip": 0, "seam_reference": 0, "head_hip": 0, "head_reference": 0}


def tile(C, k):
    """output columns per workgroup (``ddsp_hip_resblock1_tile``): the tests place T around its multiples"""
    return int(_ffi.lib().ddsp_hip_resblock1_tile(C, k))


def wide_tile(C, k):
    """output columns per workgroup of the wide form (``ddsp_hip_resblock1_wide_tile``): 128 for every k"""
    return int(_ffi.lib().ddsp_hip_resblock1_wide_tile(C, k))


def _flat(weights):
    return [t for pair in weights for t in pair]


def _pack(dims, flat):
    """the host table of one block's ``(w1, b1, w2, b2)`` per pair, for ``packed_table``"""
    (C, k), pairs, lib = dims, len(flat) // 4, _ffi.lib()
    wide = C in WIDE_CHANNELS
    nbytes = int((lib.ddsp_hip_resblock1_wide_pack_bytes if wide else lib.ddsp_hip_resblock1_pack_bytes)(C, k, pairs))
    if nbytes == 0:
        raise ValueError("resblock1: C = %d, k = %d, %d pairs is outside the kernel's range" % (C, k, pairs))
    with torch.no_grad():
        w = torch.stack([t.detach().to("cpu", torch.float32) for t in flat[0::2]]).contiguous()
        b = torch.stack([t.detach().to("cpu", torch.float32) for t in flat[1::2]]).contiguous()
    host = torch.empty(nbytes // 4, dtype=torch.float32)
    entry = lib.ddsp_hip_resblock1_wide_pack if wide else lib.ddsp_hip_resblock1_pack
    _ffi.check(entry(w.data_ptr(), b.data_ptr(), C, k, pairs, host.data_ptr(), nbytes))
    return host


def _workspace(nbytes, x):
    """the hand-over buffer between pairs, of ``x``'s device and the caller's stream there, by ``_modules.stream_workspace``'s
    rule: never shared between streams, and during a graph capture neither read nor grown (the buffer then belongs to the graph)"""
    return stream_workspace(_WS, (nbytes + 3) // 4, x, _WS_MAX)


def release_workspace():
    """drop the cached hand-over buffers of every device and stream (2 [B, C, T] activations each at the largest shape seen)"""
    drop_workspaces(_WS)


def shape_ok(C, k, dilations):
    """what the kernel takes: the x image of a tile, C rows of 128 + (k - 1) d columns padded to 16 mod 32, within 64 KB"""
    if C not in CHANNELS or k not in KERNEL_SIZES or not 1 <= len(dilations) <= 8:
        return False
    return all(int(d) >= 1 and C * ((112 + (k - 1) * int(d) + 31) // 32 * 32 + 16) <= 16384 for d in dilations)


def wide_shape_ok(C, k, dilations):
    """what the wide form takes: C in {128, 256}, and a 64-channel chunk of the x image, 64 rows of 128 + (k - 1) d columns
    padded to 16 mod 32, within 64 KB -- d <= 11 at k = 11, 18 at 7, 56 at 3"""
    if C not in WIDE_CHANNELS or k not in KERNEL_SIZES or not 1 <= len(dilations) <= 8:
        return False
    return all(int(d) >= 1 and 64 * ((112 + (k - 1) * int(d) + 31) // 32 * 32 + 16) <= 16384 for d in dilations)


def resblock1(x, weights, dilations, acc=None, scale=None, out=None):
    """``ResBlock1.forward`` on the HIP kernel: ``x [B, C, T]`` float32, ``weights`` one ``(w1 [C, C, k], b1 [C], w2, b2)`` per
    pair, ``dilations`` conv 1's dilation per pair.  Returns ``(acc + block(x)) / scale``: ``acc`` (optional, same shape) may
    be ``out``; ``scale`` None means no division.  No synchronisation; the only allocation is the result (when ``out`` is
    None) once the weight table and the hand-over buffer of this shape exist.  C in {16, 32, 64} runs the fused pair kernel
    (csrc/resblock.h), C in {128, 256} the wide form (csrc/resblock_wide.h); whatever ``ROUTE_WIDE`` says: that is the hooks'."""
    _ffi.check_device(x, acc, out)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError("resblock1: x must be a float32 [B, C, T] tensor")
    B, C, T = x.shape
    k = weights[0][0].shape[-1]
    wide = C in WIDE_CHANNELS
    if len(weights) != len(dilations) or not (wide_shape_ok if wide else shape_ok)(C, k, dilations):
        raise ValueError("resblock1: C = %d, k = %d, dilations %s is outside the kernel's range" % (C, k, tuple(dilations)))
    for w1, b1, w2, b2 in weights:
        if tuple(w1.shape) != (C, C, k) or tuple(w2.shape) != (C, C, k) or tuple(b1.shape) != (C,) or tuple(b2.shape) != (C,):
            raise ValueError("resblock1: weights must be [C, C, k] and biases [C]")
    if T < 1:
        raise ValueError("resblock1: T must be positive")
    x = x.contiguous()
    y = torch.empty_like(x) if out is None else out
    if acc is not None and (acc.shape != x.shape or acc.dtype != torch.float32 or not acc.is_contiguous()):
        raise ValueError("resblock1: acc must be a contiguous float32 tensor of x's shape")
    if not y.is_contiguous() or y.shape != x.shape or y.dtype != torch.float32:
        raise ValueError("resblock1: out must be a contiguous float32 tensor of x's shape")
    if B == 0:
        return y
    lib = _ffi.lib()
    table = packed_table("resblock_wide" if wide else "resblock", (C, k), _flat(weights), x.device, _pack)
    pairs = len(dilations)
    nws = int((lib.ddsp_hip_resblock1_wide_workspace_bytes if wide else lib.ddsp_hip_resblock1_workspace_bytes)(B, C, T, pairs))
    ws = _workspace(nws, x) if nws else None          # its real size goes to the library, which refuses one too small
    dil = (ctypes.c_int * pairs)(*[int(d) for d in dilations])
    CALLS["hip"] += 1
    entry = lib.ddsp_hip_resblock1_wide if wide else lib.ddsp_hip_resblock1
    _ffi.check(entry(x.data_ptr(), y.data_ptr(), table.data_ptr(), table.numel() * 4, B, C, T, k, ctypes.addressof(dil), pairs,
                     _ffi.ptr(acc), 0.0 if scale is None else float(scale), _ffi.ptr(ws), 0 if ws is None else ws.numel() * 4,
                     _ffi.stream_of(x)))
    return y


def mrf_stage(x, blocks):
    """one stage's ``xs = block_0(x); xs += block_j(x); xs / len(blocks)`` with ``blocks`` a list of ``(weights, dilations)``:
    the running sum is the epilogue's ``acc`` (in place), the division the last block's ``scale``"""
    xs = None
    for j, (weights, dilations) in enumerate(blocks):
        xs = resblock1(x, weights, dilations, acc=xs, scale=len(blocks) if j == len(blocks) - 1 else None, out=xs)
    return xs


def seam_tile(Cout, u):
    """input columns per workgroup of the seam (``ddsp_hip_upsample_stage_tile``)"""
    return int(_ffi.lib().ddsp_hip_upsample_stage_tile(Cout, u))


def head_tile(C):
    """outputs per workgroup of the head (``ddsp_hip_output_head_tile``)"""
    return int(_ffi.lib().ddsp_hip_output_head_tile(C))


def _pack_seam(dims, tensors):
    """the host table of a seam's ``(up weight, up bias, noise weight, noise bias)``, for ``packed_table``"""
    lib = _ffi.lib()
    nbytes = int(lib.ddsp_hip_upsample_stage_pack_bytes(*dims))
    if nbytes == 0:
        raise ValueError("upsample_stage: Cout = %d, u = %d, s = %d is outside the kernel's range" % dims)
    with torch.no_grad():
        staged = [t.detach().to("cpu", torch.float32).contiguous() for t in tensors]
    host = torch.empty(nbytes // 4, dtype=torch.float32)
    _ffi.check(lib.ddsp_hip_upsample_stage_pack(*[t.data_ptr() for t in staged], *dims, host.data_ptr(), nbytes))
    return host


def seam_shape_ok(Cin, Cout, u, s):
    return Cout in CHANNELS and Cin == 2 * Cout and u in UPSAMPLE_RATES and s in NOISE_STRIDES


def upsample_stage(x, up_weight, up_bias, stride, source, noise_weight, noise_bias, noise_stride, out=None):
    """``ConvTranspose1d(lrelu(x, 0.1)) + noise_conv(source)`` of one stage on the HIP kernel: ``x [B, 2 Cout, Tin]`` float32,
    ``up_weight [2 Cout, Cout, 2 stride]`` (ConvTranspose1d's order), ``source [B, 1, noise_stride stride Tin]`` (or without the
    channel axis), ``noise_weight [Cout, 1, 2 noise_stride]`` (``[Cout, 1, 1]`` at ``noise_stride`` 1).  Returns ``[B, Cout,
    stride Tin]``.  No synchronisation; the only allocation is the result (when ``out`` is None) once the weight table exists."""
    _ffi.check_device(x, source, out)
    if x.dtype != torch.float32 or x.dim() != 3 or source.dtype != torch.float32:
        raise ValueError("upsample_stage: x must be a float32 [B, C, T] tensor and source float32")
    B, Cin, Tin = x.shape
    u, s = int(stride), int(noise_stride)
    Cout = up_weight.shape[1] if up_weight.dim() == 3 else -1
    if not seam_shape_ok(Cin, Cout, u, s):
        raise ValueError("upsample_stage: %d -> %d channels, stride %d, noise stride %d is outside the kernel's range"
                         % (Cin, Cout, u, s))
    ks = 2 * s if s > 1 else 1
    if (tuple(up_weight.shape) != (Cin, Cout, 2 * u) or tuple(up_bias.shape) != (Cout,)
            or tuple(noise_weight.shape) != (Cout, 1, ks) or tuple(noise_bias.shape) != (Cout,)):
        raise ValueError("upsample_stage: weights must be [2 Cout, Cout, 2 u], [Cout], [Cout, 1, 2 s or 1], [Cout]")
    if Tin < 1:
        raise ValueError("upsample_stage: Tin must be positive")
    Tout = u * Tin
    if source.shape[0] != B or source.numel() != B * s * Tout or source.shape[-1] != s * Tout:
        raise ValueError("upsample_stage: source must hold %d samples per utterance" % (s * Tout))
    x, source = x.contiguous(), source.contiguous()
    y = torch.empty((B, Cout, Tout), dtype=torch.float32, device=x.device) if out is None else out
    if not y.is_contiguous() or tuple(y.shape) != (B, Cout, Tout) or y.dtype != torch.float32:
        raise ValueError("upsample_stage: out must be a contiguous float32 [B, Cout, u Tin] tensor")
    if B == 0:
        return y
    table = packed_table("seam", (Cout, u, s), (up_weight, up_bias, noise_weight, noise_bias), x.device, _pack_seam)
    CALLS["seam_hip"] += 1
    _ffi.check(_ffi.lib().ddsp_hip_upsample_stage(x.data_ptr(), source.data_ptr(), y.data_ptr(), table.data_ptr(),
                                                  table.numel() * 4, B, Cout, Tin, u, s, _ffi.stream_of(x)))
    return y


def output_head(x, weight, bias, slope=HEAD_SLOPE, out=None):
    """``tanh(conv1d(lrelu(x, slope), weight, bias, padding=3))`` on the HIP kernel: ``x [B, C, T]`` float32, ``weight [1, C, 7]``
    and ``bias [1]`` float32 on x's device -- the kernel reads them where they are, so there is no table to pack or cache.
    Returns ``[B, 1, T]``.  No synchronisation, no allocation but the result."""
    _ffi.check_device(x, weight, bias, out)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError("output_head: x must be a float32 [B, C, T] tensor")
    B, C, T = x.shape
    if C not in CHANNELS:
        raise ValueError("output_head: C = %d is outside the kernel's range" % C)
    if (tuple(weight.shape) != (1, C, HEAD_TAPS) or tuple(bias.shape) != (1,) or weight.dtype != torch.float32
            or bias.dtype != torch.float32 or weight.device != x.device or bias.device != x.device):
        raise ValueError("output_head: weight must be float32 [1, C, 7] and bias [1] on x's device")
    if T < 1:
        raise ValueError("output_head: T must be positive")
    x, weight = x.contiguous(), weight.detach().contiguous()
    y = torch.empty((B, 1, T), dtype=torch.float32, device=x.device) if out is None else out
    if not y.is_contiguous() or tuple(y.shape) != (B, 1, T) or y.dtype != torch.float32:
        raise ValueError("output_head: out must be a contiguous float32 [B, 1, T] tensor")
    if B == 0:
        return y
    CALLS["head_hip"] += 1
    _ffi.check(_ffi.lib().ddsp_hip_output_head(x.data_ptr(), weight.data_ptr(), bias.detach().data_ptr(), float(slope),
                                               y.data_ptr(), B, C, T, _ffi.stream_of(x)))
    return y


# ---- the reference's modules --------------------------------------------------------------------------------------------------

def _plain_conv(c, C, k, d):
    """a Conv1d the kernel can stand in for: C -> C channels, k taps, dilation d, 'same' zero padding, a bias, and a ``weight``
    that is a plain parameter (no weight-norm hook or parametrization left on it)"""
    return (isinstance(c, torch.nn.Conv1d) and plain(c) and c.in_channels == C and c.out_channels == C and c.kernel_size == (k,)
            and c.stride == (1,) and c.dilation == (d,) and c.groups == 1 and c.padding_mode == "zeros"
            and pad_of(c) == ((k * d - d) // 2,) and c.bias is not None)


def _block_spec(block):
    """``(weights, dilations)`` of a ResBlock1-shaped module (``convs1`` / ``convs2`` ModuleLists), or None"""
    c1s, c2s = getattr(block, "convs1", None), getattr(block, "convs2", None)
    if c1s is None or c2s is None or len(c1s) != len(c2s) or len(c1s) == 0:
        return None
    c0 = c1s[0]
    if not isinstance(c0, torch.nn.Conv1d):
        return None
    C, k = c0.in_channels, c0.kernel_size[0]
    dil = [c.dilation[0] if isinstance(c, torch.nn.Conv1d) else 0 for c in c1s]
    if not shape_ok(C, k, dil) and not (ROUTE_WIDE and wide_shape_ok(C, k, dil)):
        return None
    if not all(_plain_conv(a, C, k, d) and _plain_conv(b, C, k, 1) for a, b, d in zip(c1s, c2s, dil)):
        return None
    return [(a.weight, a.bias, b.weight, b.bias) for a, b in zip(c1s, c2s)], dil


def hip_eligible(block, x):
    """the ``(weights, dilations)`` to run ``block`` on ``x`` with the HIP kernel, or None: the reference's forward"""
    if not on_device(x, 3) or x.shape[-1] < 1 or autocast_on(x):
        return None
    spec = _block_spec(block)
    if spec is None or x.shape[1] != spec[0][0][0].shape[0]:
        return None
    if needs_grad([x] + _flat(spec[0])) or torch_faster(TORCH_FASTER, (x.shape[1], spec[0][0][0].shape[-1]), x.shape[-1]):
        return None
    return spec


def _reference_block_forward(block, x):
    CALLS["reference"] += 1

    def conv_chain(x):                                 # a stand-in class without a forward of its own: the same chain
        for c1, c2 in zip(block.convs1, block.convs2):
            x = c2(F.leaky_relu(c1(F.leaky_relu(x, LRELU_SLOPE)), LRELU_SLOPE)) + x
        return x
    return run_reference(block, conv_chain, x)


def resblock_forward(block, x):
    """the dispatcher bound as ``ResBlock1.forward``"""
    spec = hip_eligible(block, x)
    if spec is None:
        return _reference_block_forward(block, x)
    return resblock1(x, spec[0], spec[1])


def stage_forward(blocks, x):
    """the blocks of one stage, summed and divided by their number: through ``mrf_stage`` when every one is eligible,
    otherwise block by block as the reference sums them"""
    specs = [hip_eligible(b, x) for b in blocks]
    if all(s is not None for s in specs):
        return mrf_stage(x, specs)
    xs = None
    for b in blocks:
        r = b(x)
        xs = r if xs is None else xs.add_(r)
    return xs / len(blocks)


def _plain_module(c, cls):
    """a module of class ``cls`` whose ``weight`` and bias are plain float32, with zero padding, one group, no dilation and no hook"""
    return (isinstance(c, cls) and plain(c) and c.groups == 1 and c.dilation == (1,) and c.padding_mode == "zeros"
            and c.bias is not None and c.bias.dtype == torch.float32)


def _seam_spec(up, noise_conv):
    """``(Cout, u, s)`` of an upsampling the kernel can stand in for, or None"""
    if not _plain_module(up, torch.nn.ConvTranspose1d) or not _plain_module(noise_conv, torch.nn.Conv1d):
        return None
    Cout, u = up.out_channels, up.stride[0]
    if (up.in_channels != 2 * Cout or up.kernel_size != (2 * u,) or pad_of(up) != (u // 2,)
            or tuple(up.output_padding) != (0,)):
        return None
    s = noise_conv.stride[0]
    if noise_conv.in_channels != 1 or noise_conv.out_channels != Cout:
        return None
    if noise_conv.kernel_size == (1,):
        if s != 1 or pad_of(noise_conv) != (0,):
            return None
    elif s < 2 or noise_conv.kernel_size != (2 * s,) or pad_of(noise_conv) != (s // 2,):
        return None
    if not seam_shape_ok(2 * Cout, Cout, u, s):
        return None
    return Cout, u, s


def seam_eligible(up, noise_conv, x, source):
    """``(Cout, u, s)`` to run ``up(lrelu(x)) + noise_conv(source)`` with the HIP kernel, or None: the torch line"""
    if not on_device(x, 3) or x.shape[-1] < 1 or autocast_on(x):
        return None
    if not isinstance(source, torch.Tensor) or source.dtype != torch.float32 or source.dim() != 3 or source.device != x.device:
        return None
    spec = _seam_spec(up, noise_conv)
    if spec is None or x.shape[1] != 2 * spec[0]:
        return None
    Cout, u, s = spec
    if tuple(source.shape) != (x.shape[0], 1, s * u * x.shape[-1]):
        return None
    if needs_grad([x, source, up.weight, up.bias, noise_conv.weight, noise_conv.bias]):
        return None
    if torch_faster(SEAM_TORCH_FASTER, (Cout, u), x.shape[-1]):
        return None
    return spec


def seam_forward(up, noise_conv, x, source):
    """one stage's ``up(lrelu(x)) + noise_conv(source)``: the HIP kernel when eligible, the reference's line otherwise"""
    spec = seam_eligible(up, noise_conv, x, source)
    if spec is None:
        CALLS["seam_reference"] += 1
        return up(F.leaky_relu(x, LRELU_SLOPE)) + noise_conv(source)
    return upsample_stage(x, up.weight, up.bias, spec[1], source, noise_conv.weight, noise_conv.bias, spec[2])


def head_eligible(conv_post, x):
    """True to run ``tanh(conv_post(lrelu(x)))`` with the HIP kernel"""
    if not on_device(x, 3) or x.shape[-1] < 1 or autocast_on(x):
        return False
    if not _plain_module(conv_post, torch.nn.Conv1d):
        return False
    C = conv_post.in_channels
    if (C not in CHANNELS or x.shape[1] != C or conv_post.out_channels != 1 or conv_post.kernel_size != (HEAD_TAPS,)
            or conv_post.stride != (1,) or pad_of(conv_post) != (3,) or conv_post.weight.device != x.device):
        return False
    if needs_grad([x, conv_post.weight, conv_post.bias]):
        return False
    return not torch_faster(HEAD_TORCH_FASTER, C, x.shape[-1])


def head_forward(conv_post, x):
    """``tanh(conv_post(lrelu(x)))``: the HIP kernel when eligible, the reference's line otherwise"""
    if not head_eligible(conv_post, x):
        CALLS["head_reference"] += 1
        return torch.tanh(conv_post(F.leaky_relu(x)))
    return output_head(x, conv_post.weight, conv_post.bias, HEAD_SLOPE)


_GENERATOR_ATTRS = ("conv_pre", "ups", "noise_convs", "resblocks", "num_kernels", "conv_post", "m_source", "upp")


def generator_forward(gen, x, f0, fallback=None):
    """``Generator.forward(x, f0)`` of a module with the reference generator's attributes (``conv_pre``, ``ups``,
    ``noise_convs``, ``resblocks``, ``num_kernels``, ``conv_post``, ``m_source``, ``upp``): the source and ``conv_pre`` as torch
    runs them, then every stage's seam and block sum and the head through the dispatchers above, each of which decides for
    itself.  The whole call goes to ``fallback(gen, x, f0)`` (None: ``type(gen).forward``) when the first block does not even
    name a ``convs1`` / ``convs2`` pair (ResBlock2), ``x`` is not a float32 tensor on the GPU, or a gradient is needed."""
    if fallback is None:
        fallback = type(gen).forward
    if any(not hasattr(gen, a) for a in _GENERATOR_ATTRS):
        return fallback(gen, x, f0)
    first = gen.resblocks[0] if len(gen.resblocks) else None
    if (getattr(first, "convs1", None) is None or getattr(first, "convs2", None) is None or not isinstance(x, torch.Tensor)
            or x.dtype != torch.float32 or not on_device(x)
            or (torch.is_grad_enabled() and any(p.requires_grad for p in gen.parameters()))):
        return fallback(gen, x, f0)
    source = gen.m_source(f0, gen.upp).transpose(1, 2)
    x = gen.conv_pre(x)
    n = gen.num_kernels
    for i, (up, noise_conv) in enumerate(zip(gen.ups, gen.noise_convs)):
        x = seam_forward(up, noise_conv, x, source)
        x = stage_forward(gen.resblocks[i * n:(i + 1) * n], x)
    return head_forward(gen.conv_post, x)


def patch_reference_generator(wide=False):
    """Route ``nsf_hifigan.models.ResBlock1.forward`` and, in ``Generator.forward`` of an importable reference checkout, each
    stage's upsampling seam, its block sum and the output head through the dispatchers above.  ``wide`` sets ``ROUTE_WIDE``: the
    128- and 256-channel blocks go to the wide form as well, under the same conditions as the narrow ones.  Idempotent (the
    last call's ``wide`` holds); returns the module."""
    global ROUTE_WIDE
    import nsf_hifigan.models as nm
    ROUTE_WIDE = bool(wide)
    ref_generator_forward = park(nm.Generator, "forward")

    def patched_forward(self, x, f0):
        return generator_forward(self, x, f0, fallback=ref_generator_forward)

    if nm.Generator.forward is ref_generator_forward:
        nm.Generator.forward = patched_forward
    if nm.ResBlock1.forward is park(nm.ResBlock1, "forward"):
        nm.ResBlock1.forward = resblock_forward
    return nm


def unpatch_reference_generator():
    """Undo ``patch_reference_generator()``; ``ROUTE_WIDE`` is off afterwards."""
    global ROUTE_WIDE
    import sys
    ROUTE_WIDE = False
    nm = sys.modules.get("nsf_hifigan.models")
    if nm is not None:
        unpark(nm.ResBlock1, "forward")
        unpark(nm.Generator, "forward")
