"""torchaudio's band-limited sinc resampling (``torchaudio.functional.resample`` / ``torchaudio.transforms.Resample``) on HIP.

The reference resamples with ``Resample(orig, new, lowpass_filter_width=128)`` in front of the unit encoder and the F0
extractors, behind the model in the GUIs' callbacks, around the enhancer and in the cascade vocoders.  torchaudio runs it as
zero padding plus a strided ``conv1d`` with an ``[n, 1, 2 width + o]`` bank; here the same sums are one f32 MFMA GEMM per
utterance over each phase's band of live taps (csrc/resample.h).  torchaudio is not a dependency: its published semantics are
restated below op for op.

  sinc_resample_kernel      the filter bank -> (kernel [n, 1, K], width), torchaudio's ``_get_sinc_resample_kernel``
  resample                  the functional form (the bank in the waveform's dtype, as torchaudio builds it)
  Resample                  the nn.Module drop-in; ``kernel`` a non-persistent buffer, ``width`` an attribute
  patch_reference_resample  rebinds ``Resample`` wherever a module bound torchaudio's

Dispatch: a float32 CUDA tensor that needs no gradient, with reduced rates the kernel covers (o, n <= 4096 and every tile's
band <= 65 536 taps: every pair the reference uses), goes to HIP.  Anything else -- host tensors, float64, a bank built with
``dtype=``, tensors that need a gradient, rates out of range -- takes torchaudio's op sequence, which is differentiable.
"""
import math
import threading

import torch

from . import _ffi

DEFAULT_KAISER_BETA = 14.769656459379492
_METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")
_ALIASES = {"sinc_interpolation": "sinc_interp_hann", "kaiser_window": "sinc_interp_kaiser"}


def sinc_resample_kernel(orig_freq, new_freq, gcd=None, lowpass_filter_width=6, rolloff=0.99,
                         resampling_method="sinc_interp_hann", beta=None, device=torch.device("cpu"), dtype=None):
    """torchaudio's ``_get_sinc_resample_kernel``: returns ``(kernel [n, 1, 2 width + o], width)`` with o, n the rates reduced by
    their gcd.  The ops and their order are torchaudio's, including the phase offsets ``arange(0, -n, -1) / n`` taken as int64 / int
    (a float32 quotient) when ``dtype`` is None; the bank is built in float64 and cast to float32 then."""
    if not (int(orig_freq) == orig_freq and int(new_freq) == new_freq):
        raise Exception("Frequencies must be of integer type to ensure quality resampling computation.")
    if resampling_method in _ALIASES:
        resampling_method = _ALIASES[resampling_method]
    elif resampling_method not in _METHODS:
        raise ValueError("Invalid resampling method: {}".format(resampling_method))
    if gcd is None:
        gcd = math.gcd(int(orig_freq), int(new_freq))
    orig_freq = int(orig_freq) // gcd
    new_freq = int(new_freq) // gcd
    if lowpass_filter_width <= 0:
        raise ValueError("Low pass filter width should be positive.")
    base_freq = min(orig_freq, new_freq)
    base_freq *= rolloff
    width = math.ceil(lowpass_filter_width * orig_freq / base_freq)
    idx_dtype = dtype if dtype is not None else torch.float64
    idx = torch.arange(-width, width + orig_freq, dtype=idx_dtype, device=device)[None, None] / orig_freq
    t = torch.arange(0, -new_freq, -1, dtype=dtype, device=device)[:, None, None] / new_freq + idx
    t *= base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    if resampling_method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    else:
        if beta is None:
            beta = DEFAULT_KAISER_BETA
        beta_tensor = torch.tensor(float(beta))
        window = torch.i0(beta_tensor * torch.sqrt(1 - (t / lowpass_filter_width) ** 2)) / torch.i0(beta_tensor)
    t *= math.pi
    scale = base_freq / orig_freq
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    if dtype is None:
        kernels = kernels.to(dtype=torch.float32)
    return kernels, width


def _apply_torch(waveform, o, n, kernel, width):
    """torchaudio's ``_apply_sinc_resample_kernel``: pad, strided conv1d, interleave, cut (o, n reduced)."""
    shape = waveform.size()
    num_wavs, length = math.prod(shape[:-1]), shape[-1]
    waveform = waveform.reshape(num_wavs, length)
    waveform = torch.nn.functional.pad(waveform, (width, width + o))
    resampled = torch.nn.functional.conv1d(waveform[:, None], kernel, stride=o)
    resampled = resampled.transpose(1, 2).reshape(num_wavs, -1)
    target_length = torch.ceil(torch.as_tensor(n * length / o)).long()
    resampled = resampled[..., :target_length]
    return resampled.view(shape[:-1] + resampled.shape[-1:])


class _Table:
    """The bank's device table (csrc/resample.h): built on the host once, copied to each device once, kept."""

    def __init__(self, kernel, o, n, width):
        self.o, self.n, self.width = o, n, width
        self._bank = kernel.detach().to("cpu", torch.float32).reshape(n, -1).contiguous()
        self.K = self._bank.shape[1]
        self._bytes = None                             # asked of the library on first use: host-only callers never load it
        self._host = None
        self._dev = {}
        self._lock = threading.Lock()

    @property
    def bytes(self):
        if self._bytes is None:
            self._bytes = int(_ffi.lib().ddsp_hip_resample_table_bytes(self._bank.data_ptr(), self.o, self.n, self.K))
        return self._bytes

    @property
    def ok(self):
        return self.bytes > 0

    def host(self):
        if self._host is None:
            buf = torch.empty(self.bytes, dtype=torch.uint8)
            _ffi.check(_ffi.lib().ddsp_hip_resample_table(self._bank.data_ptr(), self.o, self.n, self.K, buf.data_ptr(),
                                                          self.bytes))
            self._host = buf
        return self._host

    def on(self, device):
        t = self._dev.get(device)
        if t is None:
            with self._lock:
                t = self._dev.get(device)
                if t is None:
                    t = self._dev[device] = self.host().to(device)
        return t


def resample_hip(waveform, table):
    """``waveform [..., L]`` float32 through the HIP kernel with a prepared ``_Table``; returns a new ``[..., T]`` tensor.
    No allocation besides the output, no synchronisation."""
    _ffi.check_device(waveform)
    if waveform.dtype != torch.float32:
        raise ValueError("resample: the HIP path takes float32 (got %s)" % waveform.dtype)
    shape = waveform.shape
    B, L = math.prod(shape[:-1]), shape[-1]
    x = waveform.reshape(B, L)
    T = -(-table.n * L // table.o)
    y = torch.empty(B, T, dtype=torch.float32, device=waveform.device)
    if B and T:
        tab = table.on(waveform.device)
        # strides as they are: 0 (an expanded tensor) reads the same element again, which is what the tensor holds
        _ffi.check(_ffi.lib().ddsp_hip_resample(x.data_ptr(), x.stride(0), x.stride(1), B, L, y.data_ptr(), T, tab.data_ptr(),
                                                table.bytes, table.o, table.n, table.width, _ffi.stream_of(x)))
    return y.view(shape[:-1] + (T,))


def _hip_eligible(waveform, table):
    return (waveform.is_cuda and waveform.dtype == torch.float32 and not (torch.is_grad_enabled() and waveform.requires_grad)
            and table is not None and table.ok and waveform.dim() >= 1)


_FUNCTIONAL = {}
_FUNCTIONAL_LOCK = threading.Lock()


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann",
             beta=None):
    """``torchaudio.functional.resample``: the bank is built in the waveform's dtype on its device, as torchaudio does.  On a
    float32 GPU tensor the bank and its table are built once per (rates, filter, device) and cached.  A bank built in float32
    has no exact zeros (its window is cos(pi / 2)^2 ~ 1.9e-15 at the clamp, not 0), so the kernel runs every tap of it: more
    MFMA work than the module's float64-built bank (DESIGN.md section 7.3 has the numbers)."""
    if orig_freq <= 0.0 or new_freq <= 0.0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    if orig_freq == new_freq:
        return waveform
    gcd = math.gcd(int(orig_freq), int(new_freq))
    if waveform.is_cuda and waveform.dtype == torch.float32:
        key = (int(orig_freq), int(new_freq), float(lowpass_filter_width), float(rolloff), resampling_method,
               None if beta is None else float(beta), waveform.device)
        hit = _FUNCTIONAL.get(key)
        if hit is None:
            kernel, width = sinc_resample_kernel(orig_freq, new_freq, gcd, lowpass_filter_width, rolloff, resampling_method,
                                                 beta, waveform.device, waveform.dtype)
            o, n = int(orig_freq) // gcd, int(new_freq) // gcd
            with _FUNCTIONAL_LOCK:
                hit = _FUNCTIONAL.setdefault(key, (kernel, width, _Table(kernel, o, n, width)))
        kernel, width, table = hit
        if _hip_eligible(waveform, table):
            return resample_hip(waveform, table)
    else:
        kernel, width = sinc_resample_kernel(orig_freq, new_freq, gcd, lowpass_filter_width, rolloff, resampling_method, beta,
                                             waveform.device, waveform.dtype)
    if not waveform.is_floating_point():
        raise TypeError(f"Expected floating point type for waveform tensor, but received {waveform.dtype}.")
    return _apply_torch(waveform, int(orig_freq) // gcd, int(new_freq) // gcd, kernel, width)


class Resample(torch.nn.Module):
    """``torchaudio.transforms.Resample``: same constructor, same ``kernel`` buffer (non-persistent: absent from
    ``state_dict()``) and ``width``, same output.  A float32 GPU waveform that needs no gradient goes to the HIP kernel (the
    device table of the bank is built once per device and kept); anything else runs torchaudio's op sequence."""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6,
                 rolloff=0.99, beta=None, *, dtype=None):
        super().__init__()
        self.orig_freq = orig_freq
        self.new_freq = new_freq
        self.gcd = math.gcd(int(self.orig_freq), int(self.new_freq))
        self.resampling_method = resampling_method
        self.lowpass_filter_width = lowpass_filter_width
        self.rolloff = rolloff
        self.beta = beta
        self._table = None
        if self.orig_freq != self.new_freq:
            kernel, self.width = sinc_resample_kernel(self.orig_freq, self.new_freq, self.gcd, self.lowpass_filter_width,
                                                      self.rolloff, self.resampling_method, beta, dtype=dtype)
            self.register_buffer("kernel", kernel, persistent=False)
            if dtype is None:                          # a bank of another dtype keeps torchaudio's path
                self._table = _Table(kernel, int(orig_freq) // self.gcd, int(new_freq) // self.gcd, self.width)

    def forward(self, waveform):
        if self.orig_freq == self.new_freq:
            return waveform
        o, n = int(self.orig_freq) // self.gcd, int(self.new_freq) // self.gcd
        if self.kernel.dtype == torch.float32 and _hip_eligible(waveform, self._table):
            return resample_hip(waveform, self._table)
        if not waveform.is_floating_point():
            raise TypeError(f"Expected floating point type for waveform tensor, but received {waveform.dtype}.")
        return _apply_torch(waveform, o, n, self.kernel, self.width)


def patch_reference_resample():
    """Rebind every module-level name bound to ``torchaudio.transforms.Resample`` (``from torchaudio.transforms import
    Resample`` in ddsp/vocoder.py, gui*.py, enhancer.py, encoder/rmvpe/inference.py, diffusion/ and reflow/vocoder.py) to
    ``Resample`` here, found by identity over ``sys.modules``; torchaudio itself is left as it is, and instances created earlier
    keep their class.  Needs torchaudio imported first (the reference's own imports do that).  Idempotent: returns the
    ``(module name, attribute)`` pairs it rebound, empty on a second call."""
    import sys
    ta = sys.modules.get("torchaudio.transforms")
    orig = getattr(ta, "Resample", None) if ta is not None else None
    if orig is None or orig is Resample:
        return []
    from ._patching import rebind_everywhere
    skip = [m for name, m in list(sys.modules.items()) if name == "torchaudio" or name.startswith("torchaudio.")]
    changed = rebind_everywhere({orig: Resample}, skip=skip)
    return [(mod.__name__, name) for mod, name, _old, _new in changed]
