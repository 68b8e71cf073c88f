"""What the reference-module hooks (``nsf_generator``, ``conformer``, ``attention``, ``wavenet``, ``naive_v2``) share: the cache of
packed weight tables and the staging of a host table, the per-stream workspaces, the predicates their eligibility checks are made
of, and what the two denoiser layers (``wavenet``, ``naive_v2``) have in common: the stacked step projections, the rule that
routes a size to the split form, the tiled form or torch.  ``mel`` uses ``needs_grad``.

The cache rule: a table is found again by the device, the kind of kernel, the shape integers and the ``data_ptr`` of every
parameter tensor; it is a hit only while every tensor's ``_version`` is the one it was packed at (an in-place write packs
again); the entry keeps the tensors alive, so a ``data_ptr`` cannot come back as another tensor's; all kinds share one bound of
``_PACKED_MAX`` entries, dropped oldest first; lookup, pack and insert happen under one lock.  An inference tensor (made inside
``torch.inference_mode()``) has no ``_version``, so a write to it cannot be seen: a key that holds one is never served or stored,
its table is packed on every call (``versions_of`` is the one place that decides this and the only reader of ``_version``).
"""
import threading

import torch

from . import _ffi

_LOCK = threading.Lock()
_PACKED = {}                                           # key -> (versions, device table, the tensors kept alive)
_PACKED_MAX = 256


def tracked(*tensors):
    """none of ``tensors`` (None entries skipped) is an inference tensor: every one has a ``_version`` that shows a write"""
    return not any(t is not None and t.is_inference() for t in tensors)


def versions_of(tensors):
    """every tensor's ``_version`` -- what a cache entry is a hit by --, or None when one of them is an inference tensor, which
    has none: nothing made from such tensors is served from a cache or stored in one"""
    return tuple([t._version for t in tensors]) if tracked(*tensors) else None


def autocast_on(x):
    """autocast is enabled for ``x``'s device type: a module hook then leaves the call to the module's own forward, whose torch
    ops return autocast's dtypes (the float32 kernels would not); the functional forms compute in float32 regardless"""
    return torch.is_autocast_enabled(x.device.type)


def no_autocast(x):
    """the context in which the torch ops of a functional form (an ``addmm``, a ``linear``) stay float32 inside a caller's
    autocast region for ``x``'s device type"""
    return torch.autocast(x.device.type, enabled=False)


def packed_table(kind, dims, tensors, device, pack):
    """the float32 table on ``device`` that ``pack(dims, tensors)`` -- the caller's own function, run only when the cache misses:
    it sizes the host table with its C ``*_pack_bytes`` entry, stages its operands and fills it with its C ``*_pack`` entry --
    returns for ``tensors``; cached by the rule above"""
    versions = versions_of(tensors)
    if versions is None:
        with _LOCK:
            return pack(dims, tensors).to(device)
    key = (str(device), kind, *dims, *[t.data_ptr() for t in tensors])
    with _LOCK:
        hit = _PACKED.get(key)
        if hit is not None and hit[0] == versions:
            return hit[1]
        table = pack(dims, tensors).to(device)
        while len(_PACKED) >= _PACKED_MAX:
            _PACKED.pop(next(iter(_PACKED)))
        _PACKED[key] = (versions, table, list(tensors))
    return table


def clear_packed():
    """drop every cached table"""
    with _LOCK:
        _PACKED.clear()


def pack_host(nbytes, refusal, tensors, entry, dims):
    """the host table that a caller's ``pack`` returns: ``nbytes`` is what its C ``*_pack_bytes`` entry answered (0: ValueError
    with ``refusal``), ``tensors`` are staged as contiguous CPU float32, and ``entry``, its C ``*_pack``, fills the table from the
    staged pointers, ``dims`` (with whatever further pointers the entry takes in front), the table and its size"""
    if nbytes == 0:
        raise ValueError(refusal)
    with torch.no_grad():
        staged = [t.detach().to("cpu", torch.float32).contiguous() for t in tensors]
    host = torch.empty(nbytes // 4, dtype=torch.float32)
    _ffi.check(entry(*[t.data_ptr() for t in staged], *dims, host.data_ptr(), nbytes))
    return host


_STACKED = {}                                          # data_ptrs of the projections -> (versions, W [n C, C], b [n C], kept)
_STACKED_MAX = 32                                      # for both denoisers: as many as the 16 each of them kept on its own


def stacked_projection(projs):
    """``(W [n C, C], b [n C])``: the layers' ``(weight [C, C] or [C, C, 1], bias [C])`` step projections stacked, cached by the
    rule of ``packed_table`` (found again by every tensor's ``data_ptr``, a hit while every ``_version`` is unchanged, the entry
    keeps the tensors alive, ``_STACKED_MAX`` entries dropped oldest first, under the same lock; stacked on every call, never
    stored, when one of them is an inference tensor)"""
    flat = [t for p in projs for t in p]

    def stack():
        with torch.no_grad():
            return (torch.cat([p[0].detach().reshape(p[0].shape[0], -1) for p in projs], 0).contiguous(),
                    torch.cat([p[1].detach() for p in projs], 0).contiguous())
    versions = versions_of(flat)
    if versions is None:
        return stack()
    key = tuple(t.data_ptr() for t in flat)
    with _LOCK:
        hit = _STACKED.get(key)
        if hit is not None and hit[0] == versions:
            return hit[1], hit[2]
        W, b = stack()
        while len(_STACKED) >= _STACKED_MAX:
            _STACKED.pop(next(iter(_STACKED)))
        _STACKED[key] = (versions, W, b, flat)
    return W, b


def step_biases(s, projs):
    """``d [n, B, C]``: the step embedding ``s [B, C]`` through all n layers' projections in ONE matmul"""
    W, b = stacked_projection(projs)
    with no_autocast(s):
        return torch.addmm(b, s, W.t()).view(s.shape[0], len(projs), W.shape[1]).transpose(0, 1).contiguous()


_WS_LOCK = threading.Lock()


def stream_workspace(cache, floats, x, keep):
    """the float32 buffer of at least ``floats`` elements that ``cache`` (a module's own ``OrderedDict``) holds for ``x``'s device
    and the caller's current stream there: never shared between streams (the launches of one call write and read it on that
    stream), grown on demand, the ``keep`` most recently used kept.  A buffer is allocated while its stream is the current one,
    so the caching allocator hands its memory on only to later work of that same stream: a buffer that growth, the bound or
    ``drop_workspaces`` drops while launches still use it is reused behind them, never beside them.
    During a graph capture the cache is neither read nor grown: the buffer then comes from the graph's pool and belongs to the
    graph, which holds no address that a later growth or ``drop_workspaces`` frees."""
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        return torch.empty(floats, dtype=torch.float32, device=x.device)
    key = (str(x.device), _ffi.stream_of(x))
    with _WS_LOCK:
        ws = cache.get(key)
        if ws is None or ws.numel() < floats:
            ws = cache[key] = torch.empty(floats, dtype=torch.float32, device=x.device)
            while len(cache) > keep:
                cache.popitem(last=False)
        cache.move_to_end(key)
    return ws


def drop_workspaces(cache):
    """empty a ``stream_workspace`` cache"""
    with _WS_LOCK:
        cache.clear()


def on_device(x, dim=None):
    """``x`` is where ``_ffi.check_device`` wants it; with ``dim``, it is a float32 tensor of that many dimensions as well"""
    if dim is not None and (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != dim):
        return False
    try:
        _ffi.check_device(x)                           # looked up at call time: the emulator legs of the tests replace it
    except RuntimeError:
        return False
    return True


def needs_grad(tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def pad_of(conv):
    return tuple(conv.padding) if isinstance(conv.padding, (tuple, list)) else (conv.padding,)


def plain(module):
    """``weight`` is a plain float32 parameter and the module carries no hook (a weight-norm hook recomputes ``weight``; any other
    expects the module's own forward to run); neither it nor a bias is an inference tensor (a module built or loaded inside
    ``inference_mode`` runs its own forward: cheaper than a table packed and copied to the device on every call).  What else a
    call site asks of the bias it asks itself."""
    return (isinstance(module._parameters.get("weight"), torch.Tensor) and not module._forward_pre_hooks
            and not module._forward_hooks and module.weight.dtype == torch.float32
            and tracked(module.weight, module._parameters.get("bias")))


def plain_with_bias(module):
    """``plain`` and a bias that is a plain float32 parameter too"""
    return plain(module) and isinstance(module._parameters.get("bias"), torch.Tensor) and module.bias.dtype == torch.float32


def pointwise(c, cin, cout):
    """an unpadded ``Conv1d(cin, cout, 1)``, ``plain_with_bias``"""
    return (isinstance(c, torch.nn.Conv1d) and plain_with_bias(c) and c.in_channels == cin and c.out_channels == cout
            and c.kernel_size == (1,) and c.stride == (1,) and c.dilation == (1,) and c.groups == 1 and pad_of(c) == (0,))


def torch_faster(table, key, size):
    """``table`` (a ``*_TORCH_FASTER``) lists ``key`` with a bound above ``size``, or with None: the torch chain at every size"""
    return key in table and (table[key] is None or size < table[key])


# ---- the two forms of a denoiser layer (wavenet, naive_v2) --------------------------------------------------------------------

SPLIT_TILE = 16                                        # frames per workgroup of a split form
SPLIT_MAX_TILES = 4096                                 # a split form takes B ceil(n / 16) up to here
FORMS = ("tiled", "split")


def split_in_range(B, n):
    """a split form takes ``B ceil(n / SPLIT_TILE)`` tiles up to ``SPLIT_MAX_TILES``"""
    return B * -(-n // SPLIT_TILE) <= SPLIT_MAX_TILES


def choose_form(split_below, faster, key, B, n):
    """where a hook sends a layer call of ``B x n`` frames: ``"split"`` within the split form's range below the measured
    ``split_below[key]``, else ``"tiled"`` unless ``faster`` (a ``*_TORCH_FASTER``) gives the size to torch, else None (the torch
    chain).  The two forms give the same bits, so the choice never shows in a result."""
    if key in split_below and split_in_range(B, n) and B * n < split_below[key]:
        return "split"
    return None if torch_faster(faster, key, B * n) else "tiled"

