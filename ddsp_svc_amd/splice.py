"""The real-time caller's splice of consecutive output blocks on HIP (gui.py:431-456 and ``phase_vocoder``, gui.py:15-32).

After the model and the resampler, every audio callback of the GUIs finds the offset of the new block that best lines up with the
previous block's tail (SOLA, synchronised overlap-add), crossfades the two -- linearly or through the phase vocoder -- and keeps
the new tail for the next call.  Here that is 2 launches (3 with the vocoder, csrc/splice.h) on the caller's stream, with no
allocation in a session and no device-to-host synchronisation: the shift stays on the device.

  phase_vocoder        gui.py:15-32 on 1-D float32 GPU tensors
  sola_splice          one splice, functional (new tensors)
  StreamingSplice      the GUI's callback shape: buffers bound once, one C call per block
  patch_reference_splice   rebinds a GUI module's ``phase_vocoder`` (the inline SOLA itself is code)
"""
import torch

from . import _ffi

MAX_CROSSFADE, MAX_SEARCH = 16384, 4096


def _sizes(block_frame, crossfade_frame, sola_search_frame, last_delay_frame):
    Bf, C, S, D = (int(v) for v in (block_frame, crossfade_frame, sola_search_frame, last_delay_frame))
    if Bf < 1:
        raise ValueError("sola_splice: block_frame must be >= 1 (got %d)" % Bf)
    if D < 1:
        raise ValueError("sola_splice: last_delay_frame must be >= 1: the reference's [-X:-0] slice is empty at 0 (got %d)" % D)
    if not 1 <= C <= MAX_CROSSFADE:
        raise ValueError("sola_splice: crossfade_frame must be in 1 .. %d (got %d)" % (MAX_CROSSFADE, C))
    if not 0 <= S <= MAX_SEARCH:
        raise ValueError("sola_splice: sola_search_frame must be in 0 .. %d (got %d)" % (MAX_SEARCH, S))
    return Bf, C, S, D


def _f32_1d(t, n, what, dev):
    if t.dim() != 1 or t.numel() != n or t.dtype != torch.float32 or t.device != dev:
        raise ValueError("%s must be a float32 [%d] tensor on %s (got %s %s on %s)" % (what, n, dev, t.dtype, tuple(t.shape), t.device))
    return t.contiguous()


def _workspace(B, C, use_pv, dev):
    n = int(_ffi.lib().ddsp_hip_splice_workspace_bytes(B, C, int(bool(use_pv))))
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def phase_vocoder(a, b, fade_out, fade_in):
    """``phase_vocoder(a, b, fade_out, fade_in)`` of gui.py:15-32: the crossfade of the old tail ``a`` into the new head ``b``
    through their windowed spectra: float64 sums of float32 twiddles and cosines, the phase arguments reduced exactly in
    integers (csrc/splice.h).  1-D float32 GPU tensors
    of one length n <= 16384; returns a new tensor."""
    _ffi.check_device(a)
    if a.dim() != 1:
        raise ValueError("phase_vocoder: a must be 1-D (got %s)" % (tuple(a.shape),))
    n = a.numel()
    if not 1 <= n <= MAX_CROSSFADE:
        raise ValueError("phase_vocoder: length must be in 1 .. %d (got %d)" % (MAX_CROSSFADE, n))
    a, b = _f32_1d(a, n, "phase_vocoder: a", a.device), _f32_1d(b, n, "phase_vocoder: b", a.device)
    fo, fi = _f32_1d(fade_out, n, "phase_vocoder: fade_out", a.device), _f32_1d(fade_in, n, "phase_vocoder: fade_in", a.device)
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    ws, need = _workspace(1, n, True, a.device)
    _ffi.check(_ffi.lib().ddsp_hip_phase_vocoder(a.data_ptr(), b.data_ptr(), fo.data_ptr(), fi.data_ptr(), n, out.data_ptr(),
                                                 ws.data_ptr(), need, _ffi.stream_of(a)))
    return out


def sola_splice(audio, sola_buffer, fade_in, fade_out, block_frame, crossfade_frame, sola_search_frame, last_delay_frame,
                use_phase_vocoder=False):
    """One splice of gui.py:431-456 -> ``(out, new_buffer, shift)``.

    ``audio [L]`` or ``[B, L]`` (float32, GPU, contiguous last dimension, L >= block + crossfade + search + delay); ``sola_buffer``
    the previous call's tail ``[C]`` / ``[B, C]`` (zeros at the start); ``fade_in`` / ``fade_out`` the caller's ``[C]`` windows,
    taken as given.  Returns new tensors: ``out [(B,) block]``, ``new_buffer [(B,) C]`` (read after the crossfade: with
    block < crossfade it holds crossfaded samples, as the reference's) and ``shift`` (int64, 0-dim or ``[B]``) on the device."""
    Bf, C, S, D = _sizes(block_frame, crossfade_frame, sola_search_frame, last_delay_frame)
    _ffi.check_device(audio)
    one = audio.dim() == 1
    a2 = audio.unsqueeze(0) if one else audio
    if a2.dim() != 2 or a2.dtype != torch.float32:
        raise ValueError("sola_splice: audio must be a float32 [L] or [B, L] tensor (got %s %s)" % (audio.dtype, tuple(audio.shape)))
    if a2.stride(-1) != 1:
        a2 = a2.contiguous()
    B, L = a2.shape
    if L < Bf + C + S + D:
        raise ValueError("sola_splice: audio holds %d samples, the splice needs block + crossfade + search + delay = %d"
                         % (L, Bf + C + S + D))
    dev = a2.device
    buf = sola_buffer.unsqueeze(0) if sola_buffer.dim() == 1 else sola_buffer
    if tuple(buf.shape) != (B, C) or buf.dtype != torch.float32 or buf.device != dev:
        raise ValueError("sola_splice: sola_buffer must be a float32 %s tensor on %s (got %s %s on %s)"
                         % ((B, C) if not one else (C,), dev, buf.dtype, tuple(sola_buffer.shape), buf.device))
    buf = buf.contiguous()
    fi, fo = _f32_1d(fade_in, C, "sola_splice: fade_in", dev), _f32_1d(fade_out, C, "sola_splice: fade_out", dev)
    out = torch.empty(B, Bf, dtype=torch.float32, device=dev)
    new_buf = torch.empty(B, C, dtype=torch.float32, device=dev)
    shift = torch.empty(B, dtype=torch.int64, device=dev)
    ws, need = _workspace(B, C, use_phase_vocoder, dev)
    _ffi.check(_ffi.lib().ddsp_hip_sola_splice(
        a2.data_ptr(), a2.stride(0) if B > 1 else L, B, L, Bf, C, S, D, buf.data_ptr(), new_buf.data_ptr(), fi.data_ptr(),
        fo.data_ptr(), int(bool(use_phase_vocoder)), out.data_ptr(), shift.data_ptr(), ws.data_ptr(), need, _ffi.stream_of(a2)), batch=B)
    if one:
        return out[0], new_buf[0], shift[0]
    return out, new_buf, shift


class StreamingSplice:
    """The splice for the real-time caller: one fixed shape, every buffer -- the two tails it ping-pongs, the workspace, the output
    block and the shift -- allocated once, so that a call is one C call (2 launches, 3 with the phase vocoder) and nothing else.

    ``__call__(audio)`` takes ``[L]`` (B = 1, as the GUI has it) or ``[B, L]`` and returns ``(out, shift)``: the session's own
    ``[(B,) block]`` output and int64 shift, which the next call overwrites.  The tail is kept inside (``sola_buffer``); ``reset()``
    zeroes it.  The numbers are those of chained ``sola_splice`` calls bit for bit.  One session per host thread / stream.

    Graphs (``torch.cuda.graph``, on the session's stream): a call reads one of the two tails and writes the other, and a
    captured call keeps that pair.  For a caller that runs once per block, capture two graphs back to back, one call each
    (one per parity), and replay them in turn, refilling the static input in place before each replay.  Capturing flips the
    session's parity as a call does, so after the two captures it is back where it started.  Do not mix eager calls with
    replays: an eager call flips the parity that the replays do not, and ``sola_buffer`` then names the wrong tail."""

    def __init__(self, B, block_frame, crossfade_frame, sola_search_frame, last_delay_frame, fade_in, fade_out,
                 use_phase_vocoder=False, device="cuda"):
        self.B = int(B)
        if self.B < 1:
            raise ValueError("StreamingSplice: B must be >= 1 (got %d)" % self.B)
        self.block_frame, self.crossfade_frame, self.sola_search_frame, self.last_delay_frame = \
            _sizes(block_frame, crossfade_frame, sola_search_frame, last_delay_frame)
        self.use_phase_vocoder = bool(use_phase_vocoder)
        dev = torch.device(device)
        Bf, C = self.block_frame, self.crossfade_frame
        fi, fo = fade_in.to(dev), fade_out.to(dev)
        self.fade_in = _f32_1d(fi, C, "StreamingSplice: fade_in", fi.device).clone()       # the caller's windows, kept as given
        self.fade_out = _f32_1d(fo, C, "StreamingSplice: fade_out", fi.device).clone()
        self._bufs = torch.zeros(2, self.B, C, dtype=torch.float32, device=dev)
        self._cur = 0
        self.out = torch.empty(self.B, Bf, dtype=torch.float32, device=dev)
        self.shift = torch.empty(self.B, dtype=torch.int64, device=dev)
        self._ws, self._need = _workspace(self.B, C, self.use_phase_vocoder, dev)
        self._lib = _ffi.lib()
        _ffi.check_device(self.out)
        self._dev = self.out.device
        self._stream = _ffi.stream_of(self.out)
        self._min_len = Bf + C + self.sola_search_frame + self.last_delay_frame
        self._ptrs = (self._bufs[0].data_ptr(), self._bufs[1].data_ptr())
        self._out1, self._shift1 = self.out[0], self.shift[0]

    @property
    def sola_buffer(self):
        """the current tail ``[B, C]`` (the session's own buffer)"""
        return self._bufs[self._cur]

    def reset(self):
        """back to the state of a new session: a zero tail"""
        self._bufs.zero_()
        self._cur = 0

    def __call__(self, audio):
        one = audio.dim() == 1
        if audio.device != self._dev or audio.dtype != torch.float32 or audio.dim() not in (1, 2) or audio.stride(-1) != 1 \
                or (one and self.B != 1) or (not one and audio.shape[0] != self.B) or audio.shape[-1] < self._min_len:
            raise ValueError("StreamingSplice: audio must be a float32 [%sL] tensor on %s with a contiguous last dimension and "
                             "L >= %d (got %s %s on %s, strides %s)" % ("" if self.B == 1 else "%d, " % self.B, self._dev,
                                                                        self._min_len, audio.dtype, tuple(audio.shape),
                                                                        audio.device, tuple(audio.stride())))
        if _ffi.stream_of(audio) != self._stream:
            raise RuntimeError("StreamingSplice: called on a stream other than the one the session was created on")
        L = audio.shape[-1]
        c = self._cur
        _ffi.check(self._lib.ddsp_hip_sola_splice(
            audio.data_ptr(), L if one or self.B == 1 else audio.stride(0), self.B, L, self.block_frame, self.crossfade_frame,
            self.sola_search_frame, self.last_delay_frame, self._ptrs[c], self._ptrs[1 - c], self.fade_in.data_ptr(),
            self.fade_out.data_ptr(), int(self.use_phase_vocoder), self.out.data_ptr(), self.shift.data_ptr(), self._ws.data_ptr(),
            self._need, self._stream), batch=self.B)
        self._cur = 1 - c
        return (self._out1, self._shift1) if one else (self.out, self.shift)


def patch_reference_splice(gui_module):
    """Rebind ``gui_module.phase_vocoder`` (gui.py / gui_diff.py / gui_reflow.py) to the HIP one for 1-D float32 GPU tensors of a
    supported length; anything else still goes to the module's own function.  Idempotent; returns the module."""
    orig = gui_module.phase_vocoder
    if getattr(orig, "_ddsp_hip_original", None) is not None:
        return gui_module

    def patched(a, b, fade_out, fade_in):
        ts = (a, b, fade_out, fade_in)
        if all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 for t in ts) \
                and 1 <= a.numel() <= MAX_CROSSFADE and all(t.shape == a.shape and t.device == a.device for t in ts):
            return phase_vocoder(a, b, fade_out, fade_in)
        return orig(a, b, fade_out, fade_in)

    patched._ddsp_hip_original = orig
    patched.__doc__ = orig.__doc__
    gui_module.phase_vocoder = patched
    return gui_module
