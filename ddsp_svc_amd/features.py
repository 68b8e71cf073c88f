"""The frame features of the real-time path on HIP, and the silence gate between them (csrc/frame_features.h).

``SvcDDSP.infer`` (gui.py:75-147) computes the volume envelope, the silence mask and the F0 track's post-processing in numpy on
the host: two round trips per audio callback for a caller whose block is on the GPU.  Here each is one launch on the caller's
stream, with no device-to-host synchronisation.

  volume             Volume_Extractor.extract (ddsp/vocoder.py:147-157), float64 sums
  silence_mask       the dilated threshold mask of gui.py:114-117, optionally upsampled as :118
  gate               ``output *= mask`` (gui.py:134) without the mask tensor
  decode_salience    to_local_average_f0 (encoder/rmvpe/utils.py:106-121), the result left on the device
  f0_track           the fill / retime / unvoiced handling of F0_Extractor.extract (ddsp/vocoder.py:104-105, :110-118, :139-143)
  StreamingFeatures  the GUI callback's fixed shape: buffers bound once, one C call per step
  patch_reference_features   rebinds the reference's pools and ``to_local_average_f0`` for float32 GPU tensors

The pools themselves (``MaskedAvgPool1d`` / ``MedianPool1d``) are in ``core``, where the reference has them.
"""
import numpy as np
import torch

from . import _ffi, core
from ._patching import park, rebind_everywhere, undo_rebound, unpark

TRACK_MODES = {"linear": 0, "nearest": 1}
N_CLASS = 360
MAX_DILATE = 64


def _int_hop(hop_size, what):
    h = int(hop_size)
    if h != hop_size:
        raise ValueError("%s: hop_size must be integral: the reference's int(n * hop) frame edges are not built here (got %r)"
                         % (what, hop_size))
    if h < 1:
        raise ValueError("%s: hop_size must be >= 1 (got %r)" % (what, hop_size))
    return h


def _rows(t, what, name):
    """a float32 [n] or [B, n] tensor -> ([B, n] with a contiguous last dimension, whether it was 1-D)"""
    if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.dtype != torch.float32:
        raise ValueError("%s: %s must be a float32 [n] or [B, n] tensor (got %s %s)"
                         % (what, name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    one = t.dim() == 1
    t2 = t.unsqueeze(0) if one else t
    if t2.stride(-1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < t2.shape[1]):
        t2 = t2.contiguous()
    return t2, one


def _ld(t2):
    return t2.stride(0) if t2.shape[0] > 1 else t2.shape[1]


def threshold_of(threshold_db):
    """the linear threshold as the reference's float32 comparison sees it: ``float32(10 ** (dB / 20))`` (gui.py:114)"""
    return float(np.float32(10 ** (float(threshold_db) / 20)))


def volume(audio, hop_size):
    """``Volume_Extractor(hop_size).extract(audio)``: ``[T]`` -> ``[F]`` or ``[B, T]`` -> ``[B, F]``, ``F = T // hop + 1``."""
    hop = _int_hop(hop_size, "volume")
    a2, one = _rows(audio, "volume", "audio")
    B, T = a2.shape
    if T <= (hop + 1) // 2:
        raise ValueError("volume: the reflection of hop %d needs more than %d samples (got %d)" % (hop, (hop + 1) // 2, T))
    _ffi.check_device(a2)
    out = torch.empty(B, T // hop + 1, dtype=torch.float32, device=a2.device)
    _ffi.check(_ffi.lib().ddsp_hip_volume(a2.data_ptr(), _ld(a2), B, T, hop, out.data_ptr(), _ffi.stream_of(a2)), batch=B)
    return out[0] if one else out


def _gate_sizes(block_size, dilate, what):
    block, d = int(block_size), int(dilate)
    if block != block_size or block < 1:
        raise ValueError("%s: block_size must be an integer >= 1 (got %r)" % (what, block_size))
    if not 0 <= d <= MAX_DILATE:
        raise ValueError("%s: dilate must be in 0 .. %d (got %r)" % (what, MAX_DILATE, dilate))
    return block, d


def gate(signal, volume, threshold_db, block_size, dilate=4, out=None):
    """``signal * mask`` with the mask of gui.py:114-118 (``volume > 10^(dB/20)``, a running maximum over ``2 dilate + 1`` frames,
    ``upsample`` by ``block_size``), which is never materialised.  ``signal [F block]`` / ``[B, F block]`` and ``volume [F]`` /
    ``[B, F]`` float32; ``out`` may be ``signal`` (in place) or another tensor of its shape; returns ``out``."""
    block, d = _gate_sizes(block_size, dilate, "gate")
    v2, _ = _rows(volume, "gate", "volume")
    if not isinstance(signal, torch.Tensor) or signal.dim() not in (1, 2) or signal.dtype != torch.float32:
        raise ValueError("gate: signal must be a float32 [n] or [B, n] tensor (got %s %s)"
                         % (getattr(signal, "dtype", type(signal)), tuple(getattr(signal, "shape", ()))))
    B, F = v2.shape
    if F < 1:
        raise ValueError("gate: volume holds no frame")
    want = (F * block,) if signal.dim() == 1 else (B, F * block)
    if tuple(signal.shape) != want or (signal.dim() == 1 and B != 1) or signal.device != v2.device:
        raise ValueError("gate: signal must be [%sframes * block_size = %d] on %s for volume %s (got %s on %s)"
                         % ("" if B == 1 else "%d, " % B, F * block, v2.device, tuple(volume.shape), tuple(signal.shape),
                            signal.device))
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=signal.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != want or out.dtype != torch.float32 or out.device != signal.device:
        raise ValueError("gate: out must be a float32 %s tensor on %s (got %s %s on %s)"
                         % (want, signal.device, getattr(out, "dtype", None), tuple(getattr(out, "shape", ())),
                            getattr(out, "device", None)))
    s2 = signal.unsqueeze(0) if signal.dim() == 1 else signal
    o2 = out.unsqueeze(0) if out.dim() == 1 else out
    for t, name in ((s2, "signal"), (o2, "out")):
        if t.stride(-1) != 1 or (B > 1 and t.stride(0) < F * block):
            raise ValueError("gate: %s must have a contiguous last dimension and rows that do not overlap (strides %s)"
                             % (name, tuple(t.stride())))
    _ffi.check_device(s2, v2, o2)
    v2 = v2.contiguous()
    _ffi.check(_ffi.lib().ddsp_hip_gate(s2.data_ptr(), _ld(s2), v2.data_ptr(), B, F, block, threshold_of(threshold_db), d, o2.data_ptr(), _ld(o2), _ffi.stream_of(s2)), batch=B)
    return out


def silence_mask(volume, threshold_db, block_size=None, dilate=4):
    """The frame mask of gui.py:114-116 (float32 zeros and ones, the shape of ``volume``) or, with ``block_size``, the reference's
    upsampled ``[(B,) F block]`` mask of gui.py:118, for callers that want the tensor: the gate applied to ones."""
    block, _ = _gate_sizes(1 if block_size is None else block_size, dilate, "silence_mask")
    v2, one = _rows(volume, "silence_mask", "volume")
    ones = torch.ones(v2.shape[0], v2.shape[1] * block, dtype=torch.float32, device=v2.device)
    m = gate(ones, v2, threshold_db, block, dilate, out=ones)
    return m[0] if one else m


def decode_salience(hidden, thred=0.03, center=None):
    """``to_local_average_f0(hidden, center, thred)`` (encoder/rmvpe/utils.py:106-121) with the result left on the device:
    ``hidden [B, N, 360]`` float32 -> ``f0 [B, N]``.  The first argmax on ties; ``center [B, N]`` (or ``[B, N, 1]``, integer)
    replaces it, as a Viterbi path would."""
    if not isinstance(hidden, torch.Tensor) or hidden.dim() != 3 or hidden.shape[-1] != N_CLASS or hidden.dtype != torch.float32:
        raise ValueError("decode_salience: hidden must be a float32 [B, N, %d] tensor (got %s %s)"
                         % (N_CLASS, getattr(hidden, "dtype", type(hidden)), tuple(getattr(hidden, "shape", ()))))
    h = hidden.contiguous()
    B, N, _ = h.shape
    c = None
    if center is not None:
        c = center.squeeze(-1) if center.dim() == 3 and center.shape[-1] == 1 else center
        if tuple(c.shape) != (B, N) or c.is_floating_point() or c.device != h.device:
            raise ValueError("decode_salience: center must be an integer [%d, %d] tensor on %s (got %s %s on %s)"
                             % (B, N, h.device, center.dtype, tuple(center.shape), center.device))
        c = c.to(torch.int64).contiguous()
    _ffi.check_device(h)
    out = torch.empty(B, N, dtype=torch.float32, device=h.device)
    _ffi.check(_ffi.lib().ddsp_hip_decode_salience(h.data_ptr(), B * N, _ffi.ptr(c), float(np.float32(thred)), out.data_ptr(),
                                                   _ffi.stream_of(h)))
    return out


def _track_args(src_period, hop_size, sample_rate, n_frames, start_frame, mode, what):
    if mode not in TRACK_MODES:
        raise ValueError("%s: mode must be one of %s (got %r)" % (what, sorted(TRACK_MODES), mode))
    period, hop, sr = float(src_period), float(hop_size), float(sample_rate)
    if not (period > 0 and hop > 0 and sr > 0):
        raise ValueError("%s: src_period, hop_size and sample_rate must be positive (got %r, %r, %r)"
                         % (what, src_period, hop_size, sample_rate))
    n, s = int(n_frames), int(start_frame)
    if n < 1 or not 0 <= s <= n:
        raise ValueError("%s: n_frames must be >= 1 and start_frame in 0 .. n_frames (got %r, %r)" % (what, n_frames, start_frame))
    return period, hop, sr, n, s, TRACK_MODES[mode]


def _track_workspace(B, N, n, dev):
    need = int(_ffi.lib().ddsp_hip_f0_track_workspace_bytes(B, N, n))
    return torch.empty(need, dtype=torch.uint8, device=dev), need


def f0_track(f0_src, src_period, hop_size, sample_rate, n_frames, start_frame=0, mode="linear", uv_interp=False, f0_min=65.0):
    """The post-processing of ``F0_Extractor.extract``: ``f0_src [N]`` / ``[B, N]`` (float32, zeros unvoiced) on a grid of
    ``src_period`` seconds -> ``[(B,) n_frames]`` on the hop grid behind ``start_frame`` zeros.  ``mode="linear"`` is the rmvpe /
    fcpe branch (fill, ``np.interp`` retime, the retimed unvoiced flag), ``"nearest"`` the crepe branch's index retime;
    ``uv_interp`` fills the zeros of the result and raises everything below ``f0_min`` to it."""
    period, hop, sr, n, s, m = _track_args(src_period, hop_size, sample_rate, n_frames, start_frame, mode, "f0_track")
    f2, one = _rows(f0_src, "f0_track", "f0_src")
    B, N = f2.shape
    if N < 1:
        raise ValueError("f0_track: f0_src holds no frame")
    _ffi.check_device(f2)
    out = torch.empty(B, n, dtype=torch.float32, device=f2.device)
    ws, need = _track_workspace(B, N, n, f2.device)
    _ffi.check(_ffi.lib().ddsp_hip_f0_track(f2.data_ptr(), _ld(f2), B, N, period, hop, sr, n, s, m, int(bool(uv_interp)),
                                            float(f0_min), out.data_ptr(), ws.data_ptr(), need, _ffi.stream_of(f2)))
    return out[0] if one else out


class StreamingFeatures:
    """The features of one real-time callback at a fixed shape: the volume, the track and the workspace are allocated once, and a
    step is one C call (one launch) and nothing else.  The numbers are those of the functional forms bit for bit.

    ``volume(audio [(B,) T])`` -> the session's ``[(B,) F]`` envelope (``F = T // hop + 1``), which ``gate_`` then reads;
    ``track(f0_src [(B,) N])`` -> the session's ``[(B,) F]`` track; ``gate_(signal [(B,) F block])`` gates the model's output in
    place with the mask of the last ``volume`` and returns it.  The returned envelope and track are the session's own buffers:
    the next call overwrites them.  One session per host thread / stream."""

    def __init__(self, B, n_samples, hop_size, n_src, src_period, sample_rate, block_size, threshold_db, dilate=4, start_frame=0,
                 mode="linear", uv_interp=False, f0_min=65.0, device="cuda"):
        self.B, self.T, self.N = int(B), int(n_samples), int(n_src)
        self.hop = _int_hop(hop_size, "StreamingFeatures")
        if self.B < 1 or self.N < 1:
            raise ValueError("StreamingFeatures: B and n_src must be >= 1 (got %d, %d)" % (self.B, self.N))
        if self.T <= (self.hop + 1) // 2:
            raise ValueError("StreamingFeatures: the reflection of hop %d needs more than %d samples (got %d)"
                             % (self.hop, (self.hop + 1) // 2, self.T))
        self.F = self.T // self.hop + 1
        self._period, self._hopf, self._sr, _, self.start_frame, self._mode = _track_args(
            src_period, hop_size, sample_rate, self.F, start_frame, mode, "StreamingFeatures")
        self.block, self.dilate = _gate_sizes(block_size, dilate, "StreamingFeatures")
        self._thr = threshold_of(threshold_db)
        self._uv, self._f0_min = int(bool(uv_interp)), float(f0_min)
        dev = torch.device(device)
        self.vol = torch.zeros(self.B, self.F, dtype=torch.float32, device=dev)
        self.f0 = torch.zeros(self.B, self.F, dtype=torch.float32, device=dev)
        self._ws, self._need = _track_workspace(self.B, self.N, self.F, dev)
        _ffi.check_device(self.vol)
        self._lib = _ffi.lib()
        self._dev = self.vol.device
        self._stream = _ffi.stream_of(self.vol)
        self._vol1, self._f01 = self.vol[0], self.f0[0]

    def _check(self, t, n, name):
        one = t.dim() == 1
        if t.device != self._dev or t.dtype != torch.float32 or t.dim() not in (1, 2) or t.stride(-1) != 1 or t.shape[-1] != n \
                or (one and self.B != 1) or (not one and (t.shape[0] != self.B or (self.B > 1 and t.stride(0) < n))):
            raise ValueError("StreamingFeatures: %s must be a float32 [%s%d] tensor on %s with a contiguous last dimension "
                             "(got %s %s on %s, strides %s)" % (name, "" if self.B == 1 else "%d, " % self.B, n, self._dev, t.dtype,
                                                                tuple(t.shape), t.device, tuple(t.stride())))
        if _ffi.stream_of(t) != self._stream:
            raise RuntimeError("StreamingFeatures: called on a stream other than the one the session was created on")
        return one, (n if one or self.B == 1 else t.stride(0))

    def volume(self, audio):
        one, ld = self._check(audio, self.T, "audio")
        _ffi.check(self._lib.ddsp_hip_volume(audio.data_ptr(), ld, self.B, self.T, self.hop, self.vol.data_ptr(), self._stream), batch=self.B)
        return self._vol1 if one else self.vol

    def track(self, f0_src):
        one, ld = self._check(f0_src, self.N, "f0_src")
        _ffi.check(self._lib.ddsp_hip_f0_track(f0_src.data_ptr(), ld, self.B, self.N, self._period, self._hopf, self._sr, self.F,
                                               self.start_frame, self._mode, self._uv, self._f0_min, self.f0.data_ptr(),
                                               self._ws.data_ptr(), self._need, self._stream))
        return self._f01 if one else self.f0

    def gate_(self, signal):
        _, ld = self._check(signal, self.F * self.block, "signal")
        _ffi.check(self._lib.ddsp_hip_gate(signal.data_ptr(), ld, self.vol.data_ptr(), self.B, self.F, self.block, self._thr,
                                           self.dilate, signal.data_ptr(), ld, self._stream), batch=self.B)
        return signal


# ---- the reference's own names --------------------------------------------------------------------------------------------------
_REBOUND = []
_PARKED = []                                             # (module, name): where an original is parked as _reference_<name>


def _gpu_f32(t, dim):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == dim


def _dispatch_pool(orig, mine):
    def pool(x, kernel_size):
        if _gpu_f32(x, 2) and isinstance(kernel_size, int) and 1 <= kernel_size <= 16 and x.shape[1] > kernel_size // 2:
            return mine(x, kernel_size)
        return orig(x, kernel_size)
    pool.__name__, pool.__doc__ = getattr(orig, "__name__", mine.__name__), getattr(orig, "__doc__", None)
    return pool


def _dispatch_decode(orig):
    def to_local_average_f0(hidden, center=None, thred=0.03):
        if _gpu_f32(hidden, 3) and hidden.shape[-1] == N_CLASS and (
                center is None or (isinstance(center, torch.Tensor) and center.is_cuda and not center.is_floating_point())):
            return decode_salience(hidden, thred, center).squeeze(0).cpu().numpy()       # the reference's return type
        return orig(hidden, center=center, thred=thred)
    to_local_average_f0.__doc__ = getattr(orig, "__doc__", None)
    return to_local_average_f0


def patch_reference_features():
    """Rebind, in an importable reference checkout, ``ddsp.core.MaskedAvgPool1d`` / ``MedianPool1d`` (and the names
    ``ddsp.vocoder`` imported) and ``to_local_average_f0`` of ``encoder.rmvpe.utils`` (and as ``encoder.rmvpe.inference`` imported
    it) to dispatchers: float32 GPU tensors of a supported shape go to the HIP kernels, with the reference's return types;
    anything else -- CPU tensors above all -- keeps the reference's own code.  The numpy-in, numpy-out pieces
    (``Volume_Extractor``, the track's post-processing) are left alone: call ``volume`` / ``f0_track`` from code that keeps its
    block on the device.  Idempotent; returns the ``(module name, attribute)`` pairs it rebound."""
    import importlib
    swapped = {}
    rcore = importlib.import_module("ddsp.core")
    importlib.import_module("ddsp.vocoder")              # so that its by-name imports exist to be rebound
    rutils = importlib.import_module("encoder.rmvpe.utils")
    importlib.import_module("encoder.rmvpe.inference")
    for mod, name, mine in ((rcore, "MaskedAvgPool1d", core.MaskedAvgPool1d), (rcore, "MedianPool1d", core.MedianPool1d),
                            (rutils, "to_local_average_f0", None)):
        orig = park(mod, name) if hasattr(mod, name) else None
        if orig is not None and getattr(mod, name) is orig:  # not swapped yet
            _PARKED.append((mod, name))
            swapped[orig] = _dispatch_decode(orig) if mine is None else _dispatch_pool(orig, mine)
    changed = rebind_everywhere(swapped) if swapped else []
    _REBOUND.extend(changed)
    return [(mod.__name__, name) for mod, name, _old, _new in changed]


def unpatch_reference_features():
    """Undo ``patch_reference_features()``: the originals are bound back where they were parked, and of the other bindings it
    changed exactly those that are still its own."""
    while _PARKED:
        unpark(*_PARKED.pop())
    undo_rebound(_REBOUND)
