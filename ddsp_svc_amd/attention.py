"""The performer attention of ``PCmer`` (``FastAttention`` / ``SelfAttention`` of ``ddsp.pcmer``: the softmax-kernel linear
attention) on HIP: csrc/performer_attention.h, two launches per call (keys, then queries), both sides' ``[N, 266]`` feature maps
kept on the CU, f32 MFMA.

  tile                          frames per workgroup (``ddsp_hip_performer_tile``)
  default_chunks                the number of key chunks a call uses when none is given (``ddsp_hip_performer_chunks``)
  fast_attention                the functional form of ``FastAttention.forward``: ``q, k, v [B, H, N, 64]``, ``projection [266, 64]``
  self_attention                the functional form of ``SelfAttention.forward``: one ``addmm`` for q, k and v, the kernel, ``to_out``
  fast_forward / self_forward   the dispatchers bound as ``FastAttention.forward`` / ``SelfAttention.forward``
  patch_reference_attention     rebinds those two in ``ddsp.pcmer`` where it imports; opt-in (``patch_reference`` leaves it)
  unpatch_reference_attention
  release_workspace             drop the cached key-partial buffers

Dispatch is decided from a module's structure, not its class.  ``fast_eligible``: ``dim_heads == 64``, a float32
``projection_matrix [266, 64]`` on q's device, not ``causal``, not ``generalized_attention``, not ``no_projection``, ``v`` given.
``self_eligible``: ``local_attn is None``, ``global_heads == heads``, four plain hook-free float32 ``nn.Linear`` with biases
(``to_q``, ``to_k``, ``to_v``: any width to ``heads * 64``), the dropout inactive, no context and no mask, and a ``fast_attention``
that is eligible itself.  Both: float32 tensors on the GPU, no gradient needed, autocast off, no weight or projection matrix that
is an inference tensor.  Everything else -- a mask, cross-attention, local heads, other head widths, training, CPU tensors, bf16 --
runs the reference's own forward.  ``normalize`` is read at call time from ``FLAG_PCMER_NORM`` of the module that defines the
class.  ``ATTN_TORCH_FASTER`` maps the head width to the number of frames B N below which the same-GPU torch chain was measured
faster (tools/attention_bench.py).
"""
import collections
import sys

import torch
import torch.nn.functional as F

from . import _ffi
from ._modules import (autocast_on, drop_workspaces, needs_grad, no_autocast, on_device, pack_host, packed_table,
                       plain_with_bias, stream_workspace, torch_faster, tracked)
from ._patching import patch_forwards, run_reference, unpatch_forwards

DIM_HEAD = 64
FEATURES = 266
# head width -> the number of frames B N below which the torch op chain was measured faster on the same GPU (None: at every
# size).  tools/attention_bench.py on one MI355X (profiles/attention_throughput.json, attention_latency.json): the kernels were
# faster at all four shapes, 1 x 100, 1 x 203, 48 x 172 and 32 x 862 frames (x2.4 .. x3.2 for the core), so nothing is listed.
ATTN_TORCH_FASTER = {}
# dispatch counters (tests and tools read them): kernel calls / calls handed to the reference's forward
CALLS = {"hip": 0, "reference": 0}
PACKS = {"count": 0}                                   # tables built: projections packed and q/k/v weights concatenated

_WS = collections.OrderedDict()                        # (device, stream) -> the key partials' buffer
_WS_MAX = 16


def tile():
    """frames per workgroup (``ddsp_hip_performer_tile``)"""
    return int(_ffi.lib().ddsp_hip_performer_tile(DIM_HEAD, FEATURES))


def default_chunks(B, H, N):
    """key chunks per (batch item, head): enough that ``B H chunks`` workgroups fill the CUs, at most ``ceil(N / tile)``"""
    return int(_ffi.lib().ddsp_hip_performer_chunks(int(B), int(H), int(N)))


def _workspace(nbytes, x):
    """the key partials' buffer of ``x``'s device and the caller's stream there, by ``_modules.stream_workspace``'s rule: never
    shared between streams, and during a graph capture neither read nor grown (the buffer then belongs to the graph)"""
    return stream_workspace(_WS, max((nbytes + 3) // 4, 4), x, _WS_MAX)


def release_workspace():
    """drop the cached key-partial buffers of every device and stream"""
    drop_workspaces(_WS)


def _pack(dims, tensors):
    """the host table of a projection matrix, for ``packed_table``"""
    lib = _ffi.lib()
    refusal = "fast_attention: (dim_head, features) = (%d, %d) is outside the kernel's range" % dims
    host = pack_host(int(lib.ddsp_hip_performer_pack_bytes(*dims)), refusal, tensors[:1], lib.ddsp_hip_performer_pack, dims)
    PACKS["count"] += 1
    return host


def _cat(dims, tensors):
    """``[wq^T | wk^T | wv^T]`` as ``[D, 3 inner]`` followed by the three biases, flat, for ``packed_table``"""
    D, inner = dims
    with torch.no_grad():
        w = torch.cat([t.detach().to(torch.float32) for t in tensors[:3]], 0).t().contiguous().reshape(-1)
        b = torch.cat([t.detach().to(torch.float32) for t in tensors[3:]], 0)
        host = torch.cat([w, b]).cpu()
    PACKS["count"] += 1
    return host


def _kernel_view(t):
    """``t [B, H, N, 64]`` as the kernel addresses it: the last dimension contiguous, strides multiples of 4 floats, 16-byte base"""
    if t.stride(3) != 1 or any(s % 4 for s in t.stride()[:3]) or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def fast_attention(q, k, v, projection, normalize=False, chunks=None, out=None):
    """``FastAttention.forward(q, k, v)`` on the HIP kernels: q, k, v float32 ``[B, H, N, 64]`` with any batch, head and frame
    strides and a contiguous last dimension (the three slices of one ``[B, N, 3 H 64]`` projection result are read in place),
    ``projection [266, 64]``, ``normalize`` = ``FLAG_PCMER_NORM``.  Returns ``[B, H, N, 64]`` as a permuted view of a ``[B, N, H,
    64]`` buffer (``out``, ``[B, N, H 64]`` or ``[B, N, H, 64]`` contiguous, when given), so ``'b h n d -> b n (h d)'`` costs no
    copy.  ``chunks`` overrides the number of key chunks.  No synchronisation; once the table and the workspace exist the only
    allocation is the result, so a call can be captured in a graph."""
    _ffi.check_device(q, k, v, projection, out)
    if any(t.dtype != torch.float32 or t.dim() != 4 for t in (q, k, v)) or not (q.shape == k.shape == v.shape):
        raise ValueError("fast_attention: q, k, v must be float32 [B, H, N, d] tensors of one shape")
    B, H, N, d = q.shape
    if projection.dim() != 2 or projection.shape[1] != d:
        raise ValueError("fast_attention: projection must be [features, d]")
    m = projection.shape[0]
    if (d, m) != (DIM_HEAD, FEATURES):
        raise ValueError("fast_attention: (dim_head, features) = (%d, %d) is outside the kernel's range" % (d, m))
    if N < 1 or H < 1:
        raise ValueError("fast_attention: H and N must be positive")
    if out is None:
        buf = torch.empty((B, N, H, d), dtype=torch.float32, device=q.device)
    else:
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * N * H * d or out.shape[:2] != (B, N):
            raise ValueError("fast_attention: out must be a contiguous float32 [B, N, H d] tensor")
        buf = out.view(B, N, H, d)
    res = buf.permute(0, 2, 1, 3)
    if B == 0:
        return res
    q, k, v = _kernel_view(q), _kernel_view(k), _kernel_view(v)
    lib = _ffi.lib()
    chunks = default_chunks(B, H, N) if chunks is None else int(chunks)
    if chunks < 1:
        raise ValueError("fast_attention: chunks must be positive")
    table = packed_table("performer", (d, m), [projection], q.device, _pack)
    need = int(lib.ddsp_hip_performer_workspace_bytes(B, H, N, chunks))
    ws = _workspace(need, q)
    strides = (_ffi.c_long * 12)(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *res.stride()[:3])
    CALLS["hip"] += 1
    _ffi.check(lib.ddsp_hip_performer_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), res.data_ptr(), strides, table.data_ptr(),
                                                table.numel() * 4, ws.data_ptr(), ws.numel() * 4, B, H, N, d, m,
                                                1 if normalize else 0, chunks, _ffi.stream_of(q)))
    return res


def self_attention(x, wq, bq, wk, bk, wv, bv, wo, bo, projection, heads=8, normalize=False):
    """``SelfAttention.forward(x)`` without context, mask or local heads: ``x [B, N, D]`` float32, the ``to_q`` / ``to_k`` /
    ``to_v`` weights ``[heads * 64, D]`` and biases, ``to_out``'s ``wo [Dout, heads * 64]``, ``bo``.  One ``addmm`` against the
    three weight matrices concatenated (cached like a packed table), the kernel on the three slices of its result, ``F.linear``
    for ``to_out``: the linear layers stay rocBLAS's."""
    _ffi.check_device(x)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError("self_attention: x must be a float32 [B, N, D] tensor")
    B, N, D = x.shape
    inner = heads * DIM_HEAD
    if any(tuple(w.shape) != (inner, D) for w in (wq, wk, wv)) or any(tuple(b.shape) != (inner,) for b in (bq, bk, bv)):
        raise ValueError("self_attention: to_q, to_k, to_v must be [heads * 64, D] with [heads * 64] biases")
    if wo.dim() != 2 or wo.shape[1] != inner:
        raise ValueError("self_attention: to_out must be [Dout, heads * 64]")
    cat = packed_table("performer_qkv", (D, inner), [wq, wk, wv, bq, bk, bv], x.device, _cat)
    w, b = cat[:D * 3 * inner].view(D, 3 * inner), cat[D * 3 * inner:]
    with no_autocast(x):                               # float32 inside a caller's autocast region too: the kernels take no other
        qkv = torch.addmm(b, x.reshape(B * N, D), w).view(B, N, 3, heads, DIM_HEAD)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        y = fast_attention(q, k, v, projection, normalize=normalize)
        return F.linear(y.permute(0, 2, 1, 3).reshape(B, N, inner), wo, bo)


# ---- the reference's modules --------------------------------------------------------------------------------------------------

def _normalize_flag(module):
    """``FLAG_PCMER_NORM`` of the module that defines ``module``'s class, now (``PCmer(pcmer_norm=True)`` sets that global)"""
    return bool(getattr(sys.modules.get(type(module).__module__), "FLAG_PCMER_NORM", False))


def _hooked(m):
    return bool(m._forward_pre_hooks or m._forward_hooks)


def _fast_spec(module, device):
    """the projection matrix of a module with ``FastAttention``'s attributes in the form the kernels take, or None"""
    if not isinstance(module, torch.nn.Module) or _hooked(module):
        return None
    proj = getattr(module, "projection_matrix", None)
    if (getattr(module, "dim_heads", None) != DIM_HEAD or not isinstance(proj, torch.Tensor) or proj.dtype != torch.float32
            or tuple(proj.shape) != (FEATURES, DIM_HEAD) or proj.device != device or not tracked(proj)):
        return None
    if getattr(module, "causal", True) or getattr(module, "generalized_attention", True) or getattr(module, "no_projection", True):
        return None
    return proj


def fast_eligible(module, q, k, v):
    """the projection matrix to run ``module`` (a ``FastAttention``) on q, k, v with the HIP kernels, or None: its own forward"""
    if v is None or not (on_device(q, 4) and on_device(k, 4) and on_device(v, 4)) or autocast_on(q):
        return None
    proj = _fast_spec(module, q.device)
    if proj is None:
        return None
    if not (q.shape == k.shape == v.shape) or q.shape[-1] != DIM_HEAD or q.shape[2] < 1 or q.shape[1] < 1:
        return None
    if k.device != q.device or v.device != q.device or needs_grad([q, k, v, proj]):
        return None
    if torch_faster(ATTN_TORCH_FASTER, DIM_HEAD, q.shape[0] * q.shape[2]):
        return None
    return proj


def _linear(m, cout=None):
    return isinstance(m, torch.nn.Linear) and plain_with_bias(m) and (cout is None or m.out_features == cout)


def self_eligible(module, x, context=None, mask=None, context_mask=None):
    """the arguments of ``self_attention`` after ``x`` to run ``module`` (a ``SelfAttention``) on the HIP kernels, or None"""
    if context is not None or mask is not None or context_mask is not None or not on_device(x, 3) or x.shape[1] < 1:
        return None
    if autocast_on(x) or not isinstance(module, torch.nn.Module) or _hooked(module):
        return None
    heads, fast = getattr(module, "heads", None), getattr(module, "fast_attention", None)
    if (not isinstance(heads, int) or heads < 1 or getattr(module, "local_attn", True) is not None
            or getattr(module, "global_heads", None) != heads or fast is None):
        return None
    lin = [getattr(module, n, None) for n in ("to_q", "to_k", "to_v", "to_out")]
    inner = heads * DIM_HEAD
    if not all(_linear(m, inner) for m in lin[:3]) or not _linear(lin[3]) or lin[3].in_features != inner:
        return None
    if any(m.in_features != x.shape[-1] for m in lin[:3]):
        return None
    drop = getattr(module, "dropout", None)
    if not isinstance(drop, torch.nn.Dropout) or _hooked(drop) or (drop.p != 0 and drop.training):
        return None
    flat = [t for m in lin for t in (m.weight, m.bias)]
    if any(t.device != x.device for t in flat) or needs_grad([x] + flat):
        return None
    proj = _fast_spec(fast, x.device)
    if proj is None or needs_grad([proj]) or torch_faster(ATTN_TORCH_FASTER, DIM_HEAD, x.shape[0] * x.shape[1]):
        return None
    return (*flat, proj)


def _reference(module, *args, **kw):
    CALLS["reference"] += 1
    return run_reference(module, None, *args, **kw)


def fast_forward(module, q, k, v):
    """the dispatcher bound as ``FastAttention.forward``"""
    proj = fast_eligible(module, q, k, v)
    if proj is None:
        return _reference(module, q, k, v)
    return fast_attention(q, k, v, proj, normalize=_normalize_flag(module))


def self_forward(module, x, context=None, mask=None, context_mask=None, **kw):
    """the dispatcher bound as ``SelfAttention.forward``"""
    spec = self_eligible(module, x, context, mask, context_mask)
    if spec is None:
        return _reference(module, x, context=context, mask=mask, context_mask=context_mask, **kw)
    return self_attention(x, *spec, heads=module.heads, normalize=_normalize_flag(module.fast_attention))


_REFERENCE_MODULES = ("ddsp.pcmer",)
_CLASSES = (("FastAttention", lambda self, q, k, v: fast_forward(self, q, k, v)),
            ("SelfAttention", lambda self, x, context=None, mask=None, context_mask=None, **kw:
             self_forward(self, x, context, mask, context_mask, **kw)))


def patch_reference_attention(modules=None):
    """Route ``FastAttention.forward`` and ``SelfAttention.forward`` of ``ddsp.pcmer`` (where it imports: it needs
    local_attention; or of the module names or objects given) through the dispatchers above.  Idempotent; returns the list of
    modules patched.  ``vocoder.patch_reference()`` does not call it: the hook is opt-in."""
    return patch_forwards(_REFERENCE_MODULES if modules is None else modules, _CLASSES)


def unpatch_reference_attention(modules=None):
    """Undo ``patch_reference_attention()``."""
    unpatch_forwards(_REFERENCE_MODULES if modules is None else modules, [name for name, _ in _CLASSES])
