"""What the reference-module hooks (``nsf_generator``, ``conformer``, ``mel``) share: the cache of packed weight tables, the
predicates their eligibility checks are made of and the rule of the per-stream workspaces (``attention``, ``naive_v2``).

The cache rule: a table is found again by the device, the kind of kernel, the shape integers and the ``data_ptr`` of every
parameter tensor; it is a hit only while every tensor's ``_version`` is the one it was packed at (an in-place write packs
again); the entry keeps the tensors alive, so a ``data_ptr`` cannot come back as another tensor's; all kinds share one bound of
``_PACKED_MAX`` entries, dropped oldest first; lookup, pack and insert happen under one lock.
"""
import threading

import torch

from . import _ffi

_LOCK = threading.Lock()
_PACKED = {}                                           # key -> (versions, device table, the tensors kept alive)
_PACKED_MAX = 256


def packed_table(kind, dims, tensors, device, pack):
    """the float32 table on ``device`` that ``pack(dims, tensors)`` -- the caller's own function, run only when the cache misses:
    it sizes the host table with its C ``*_pack_bytes`` entry, stages its operands and fills it with its C ``*_pack`` entry --
    returns for ``tensors``; cached by the rule above"""
    key = (str(device), kind, *dims, *[t.data_ptr() for t in tensors])
    versions = tuple([t._version for t in tensors])
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


_WS_LOCK = threading.Lock()


def stream_workspace(cache, floats, x, keep):
    """the float32 buffer of at least ``floats`` elements that ``cache`` (a module's own ``OrderedDict``) holds for ``x``'s device
    and the caller's current stream there: never shared between streams, grown on demand, the ``keep`` most recently used kept.
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
    expects the module's own forward to run).  What a call site asks of the bias it asks itself."""
    return (isinstance(module._parameters.get("weight"), torch.Tensor) and not module._forward_pre_hooks
            and not module._forward_hooks and module.weight.dtype == torch.float32)


def torch_faster(table, key, size):
    """``table`` (a ``*_TORCH_FASTER``) lists ``key`` with a bound above ``size``, or with None: the torch chain at every size"""
    return key in table and (table[key] is None or size < table[key])
