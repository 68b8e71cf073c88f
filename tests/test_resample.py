"""torchaudio-compatible sinc resampling (ddsp_svc_amd.resample): the bank, the HIP kernel on the emulator and the GPU against a
float64 oracle, the dispatch, the C ABI and the reference patch hook."""
import sys
import types

import numpy as np
import pytest
import torch

from tests import resample_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import resample as R  # noqa: E402

LW = 128
# the reference's own pairs (Resample(..., lowpass_filter_width=128) at every call site)
PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (32000, 16000), (40000, 16000), (24000, 16000),
         (44100, 48000), (48000, 44100),
         (44100, 46700), (44100, 58900), (44100, 88200), (46700, 44100), (58900, 44100), (88200, 44100)]
# (orig, new, lowpass_filter_width, rolloff, method)
CONFIGS = [(a, b, LW, 0.99, "sinc_interp_hann") for a, b in PAIRS] + [
    (44100, 16000, 6, 0.99, "sinc_interp_hann"),             # torchaudio's defaults
    (48000, 44100, 6, 0.99, "sinc_interp_hann"),
    (44100, 16000, LW, 0.99, "sinc_interp_kaiser"),
    (44100, 48000, 6, 0.99, "sinc_interp_kaiser"),
    (48000, 16000, LW, 0.945, "sinc_interp_hann"),
    (44100, 46700, LW, 0.945, "sinc_interp_hann"),
]
CFG_IDS = ["%d-%d-lw%d-r%g-%s" % (a, b, lw, r, m[11:]) for a, b, lw, r, m in CONFIGS]


def _module(cfg):
    a, b, lw, r, m = cfg
    return R.Resample(a, b, resampling_method=m, lowpass_filter_width=lw, rolloff=r)


def _run(mod, x, device):
    """the HIP kernel: through the module on the GPU (its dispatch), through resample_hip on the emulator"""
    if device.type == "cpu":
        return R.resample_hip(x, mod._table)
    return mod(x)


def _check(y, ref, x, what=""):
    y = y.detach().cpu().numpy().astype(np.float64)
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    yr, rr = y.reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    rms = lambda v: np.sqrt(np.mean(np.square(v), axis=-1))
    rel = rms(yr - rr) / np.maximum(rms(rr), 1e-30)
    xmax = float(np.abs(np.asarray(x.detach().cpu(), dtype=np.float64)).max()) if x.numel() else 1.0
    mx = float(np.abs(yr - rr).max())
    assert rel.max() <= 1e-6, (what, rel.max())
    assert mx <= 5e-6 * xmax, (what, mx, xmax)
    return float(rel.max())


def _no_torch_path(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("took the torch path")
    monkeypatch.setattr(R, "_apply_torch", boom)


# ---- the bank ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_bank_matches_oracle(cfg):
    a, b, lw, r, m = cfg
    k, w = R.sinc_resample_kernel(a, b, lowpass_filter_width=lw, rolloff=r, resampling_method=m)
    ko, wo, t_raw = O.bank(a, b, lw, r, m)
    o, n = O.reduced(a, b)
    assert w == wo
    assert tuple(k.shape) == (n, 1, 2 * w + o) and k.dtype == torch.float32
    k = k[:, 0].numpy()
    ulps = np.abs(k.view(np.int32).astype(np.int64) - ko.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, ulps.max()
    # closed forms: the t == 0 tap of phase 0, and (hann: its window is 0 there) every tap the clamp reached is exactly zero
    assert k[0, w] == np.float32(r * min(o, n) / o)
    if m == "sinc_interp_hann":
        assert np.all(k[np.abs(t_raw) >= lw] == 0.0)


def test_bank_dtype_and_errors():
    k, w = R.sinc_resample_kernel(44100, 16000, lowpass_filter_width=6, dtype=torch.float64)
    assert k.dtype == torch.float64 and tuple(k.shape) == (160, 1, 2 * w + 441)
    with pytest.raises(Exception):
        R.sinc_resample_kernel(44100.5, 16000)
    with pytest.raises(ValueError):
        R.sinc_resample_kernel(44100, 16000, lowpass_filter_width=0)
    with pytest.raises(ValueError):
        R.sinc_resample_kernel(44100, 16000, resampling_method="linear")
    with pytest.raises(Exception):
        R.Resample(44100.5, 16000)
    with pytest.raises(ValueError):
        R.Resample(44100, 16000, lowpass_filter_width=-1)
    with pytest.raises(ValueError):
        R.resample(torch.zeros(10), 44100, 16000, lowpass_filter_width=0)


# ---- forward against the oracle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_forward_lengths(dev, cfg, monkeypatch):
    a, b, lw, r, m = cfg
    o, n = O.reduced(a, b)
    mod = _module(cfg).to(dev)
    _no_torch_path(monkeypatch)
    ko = mod.kernel[:, 0].cpu().numpy()
    g = torch.Generator().manual_seed(a + 7 * b + lw)
    worst = 0.0
    for L in sorted({0, 1, o - 1, o, o + 1, 4999}):
        for B in (1, 3):
            x = torch.randn(B, L, generator=g).to(dev)
            y = _run(mod, x, dev)
            assert y.shape == (B, -(-n * L // o))
            worst = max(worst, _check(y, O.apply(x.cpu().numpy(), a, b, ko, mod.width), x, (L, B)))
    print("\n%d -> %d lw %d rolloff %g %s: worst relative RMS against the float64 oracle %.2e" % (a, b, lw, r, m, worst))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_forward_shapes_and_strides(dev, monkeypatch):
    cfg = CONFIGS[0]
    a, b = cfg[:2]
    mod = _module(cfg).to(dev)
    _no_torch_path(monkeypatch)
    ko = mod.kernel[:, 0].cpu().numpy()
    g = torch.Generator().manual_seed(3)
    x1 = torch.randn(3001, generator=g).to(dev)                      # [L]
    _check(_run(mod, x1, dev), O.apply(x1.cpu().numpy(), a, b, ko, mod.width), x1, "1-D")
    x3 = torch.randn(2, 3, 2222, generator=g).to(dev)                # [2, 3, L]
    y3 = _run(mod, x3, dev)
    assert y3.shape == (2, 3, -(-160 * 2222 // 441))
    _check(y3, O.apply(x3.cpu().numpy(), a, b, ko, mod.width), x3, "3-D")
    big = torch.randn(3, 2 * 2500 + 1, generator=g).to(dev)
    xs = big[:, 1::2]                                                # non-contiguous: element stride 2
    assert not xs.is_contiguous()
    _check(_run(mod, xs, dev), O.apply(xs.cpu().numpy(), a, b, ko, mod.width), xs, "strided")
    xt = torch.randn(1800, 2, generator=g).to(dev).t()               # rows of a transposed tensor
    _check(_run(mod, xt, dev), O.apply(xt.cpu().numpy(), a, b, ko, mod.width), xt, "transposed")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[2] == LW and c[3] == 0.99 and c[4] == "sinc_interp_hann"],
                         ids=lambda c: "%d-%d" % c[:2])
def test_forward_gpu_10s_batch32(cfg, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    a, b = cfg[:2]
    mod = _module(cfg).to(dev)
    _no_torch_path(monkeypatch)
    ko = mod.kernel[:, 0].cpu().numpy()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(32, 10 * 44100, generator=g)
    y = mod(x.to(dev))
    assert y.shape == (32, -(-O.reduced(a, b)[1] * x.shape[1] // O.reduced(a, b)[0]))
    sel = [0, 17, 31]                                                # the float64 oracle on three of the 32 rows
    rel = _check(y[sel], O.apply(x[sel].numpy(), a, b, ko, mod.width), x[sel], "B=32 x 10 s")
    print("\n%d -> %d, B = 32 x 10 s: relative RMS against the float64 oracle %.2e" % (a, b, rel))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_forward_expanded_inputs(dev, monkeypatch):
    """stride-0 inputs (``expand``): every element of a row, or every row, lives at one address, and the kernel reads it there"""
    cfg = CONFIGS[0]
    a, b = cfg[:2]
    mod = _module(cfg).to(dev)
    _no_torch_path(monkeypatch)
    ko = mod.kernel[:, 0].cpu().numpy()
    g = torch.Generator().manual_seed(5)
    base = (torch.arange(6000, dtype=torch.float32) * 1e-3 + 0.5).to(dev)
    cases = {
        "[L], stride 0": base[:1].expand(4000),
        "[B, L], strides (1, 0)": torch.randn(3, 1, generator=g).to(dev).expand(3, 4000),
        "[B, L], strides (0, 1)": torch.randn(4000, generator=g).to(dev).expand(3, 4000),
        "[2, 3, L], strides (0, 1, 0)": torch.randn(3, 1, generator=g).to(dev).expand(2, 3, 2500),
    }
    for what, x in cases.items():
        assert 0 in x.stride()
        _check(_run(mod, x, dev), O.apply(x.cpu().numpy(), a, b, ko, mod.width), x, what)
    y = R.resample(base[:1].expand(4000), a, b, lowpass_filter_width=LW) if dev.type == "cuda" else None
    if y is not None:                                                # the functional form on the GPU: its own float32 bank
        k32, w = R.sinc_resample_kernel(a, b, lowpass_filter_width=LW, device=dev, dtype=torch.float32)
        _check(y, O.apply(np.full(4000, 0.5), a, b, k32[:, 0].cpu().numpy(), w), base[:1], "functional")


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("pair", [(44100, 16000), (48000, 16000), (44100, 48000), (48000, 44100), (44100, 88200),
                                  (88200, 44100), (24000, 16000)], ids=lambda p: "%d-%d" % p)
def test_sine_alignment(dev, pair):
    """independent of the oracle: a sine below 0.875 of the lower Nyquist comes out as the same sine at the new rate"""
    a, b = pair
    mod = R.Resample(a, b, lowpass_filter_width=LW).to(dev)
    f = 0.875 * min(a, b) / 2 * 0.97
    L = a                                                            # 1 s: 5 % of it is wider than the filter
    x = torch.from_numpy(np.sin(2 * np.pi * f * np.arange(L) / a).astype(np.float32)).to(dev)
    y = _run(mod, x, dev).cpu().numpy().astype(np.float64)
    want = np.sin(2 * np.pi * f * np.arange(y.shape[0]) / b)
    cut = int(0.05 * y.shape[0])
    assert np.abs(y[cut:-cut] - want[cut:-cut]).max() <= 1e-4


# ---- identity, errors, buffer, dispatch -------------------------------------------------------------------------------------------

def test_identity_and_buffer():
    x = torch.randn(2, 100)
    m = R.Resample(16000, 16000)
    assert m(x) is x
    assert R.resample(x, 8000, 8000) is x
    m = R.Resample(44100, 16000, lowpass_filter_width=LW)
    assert "kernel" not in m.state_dict() and "kernel" in dict(m.named_buffers())
    assert m.width == 357 and m.kernel.shape == (160, 1, 1155)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_fallback_matches_oracle(dtype):
    a, b = 44100, 16000
    x = torch.randn(2, 3000, dtype=dtype)
    m = R.Resample(a, b, lowpass_filter_width=LW)
    ko, w, _ = O.bank(a, b, LW)
    y = m(x.float()) if dtype == torch.float32 else R.Resample(a, b, lowpass_filter_width=LW, dtype=torch.float64)(x)
    assert y.dtype == dtype
    if dtype == torch.float32:
        _check(y, O.apply(x.numpy(), a, b, ko, w), x)
    else:                                                            # a float64 bank: the oracle's float32 bank is 1e-8 off
        ref = O.apply(x.numpy(), a, b, R.sinc_resample_kernel(a, b, lowpass_filter_width=LW, dtype=torch.float64)[0][:, 0]
                      .numpy(), w)
        assert np.abs(y.numpy() - ref).max() <= 1e-10
    yf = R.resample(x, a, b, lowpass_filter_width=LW)               # the functional form: the bank in x's dtype
    assert yf.dtype == dtype and yf.shape == y.shape


def test_gradient_flows():
    x = torch.randn(2, 40, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: R.resample(v, 5, 3, lowpass_filter_width=4), (x,))
    m = R.Resample(5, 3, lowpass_filter_width=4)
    xf = torch.randn(1, 60, requires_grad=True)
    m(xf).sum().backward()
    assert xf.grad is not None and torch.isfinite(xf.grad).all()


@pytest.mark.gpu
def test_gpu_grad_takes_torch_path():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    m = R.Resample(44100, 16000, lowpass_filter_width=LW).to(dev)
    x = torch.randn(2, 5000, device=dev)
    y_hip = m(x)
    xg = x.clone().requires_grad_(True)
    called = []
    orig = R._apply_torch
    R._apply_torch = lambda *a, **k: called.append(1) or orig(*a, **k)
    try:
        y_t = m(xg)
    finally:
        R._apply_torch = orig
    assert called and y_t.requires_grad
    y_t.sum().backward()
    assert xg.grad is not None
    ko = m.kernel[:, 0].cpu().numpy()
    ref = O.apply(x.cpu().numpy(), 44100, 16000, ko, m.width)
    _check(y_hip, ref, x)
    rel = np.sqrt(np.mean((y_t.detach().cpu().numpy() - ref) ** 2)) / np.sqrt(np.mean(ref ** 2))
    assert rel <= 1e-5                                               # the vendor conv: its own summation
    with torch.no_grad():                                            # no gradient needed: HIP again
        _check(m(xg), ref, x)


@pytest.mark.gpu
def test_gpu_functional_and_float64():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    x = torch.randn(3, 7000, device=dev)
    y = R.resample(x, 48000, 16000, lowpass_filter_width=LW)
    k32, w = R.sinc_resample_kernel(48000, 16000, lowpass_filter_width=LW, device=dev, dtype=torch.float32)
    _check(y, O.apply(x.cpu().numpy(), 48000, 16000, k32[:, 0].cpu().numpy(), w), x)
    y2 = R.resample(x, 48000, 16000, lowpass_filter_width=LW)        # cached bank and table
    assert torch.equal(y, y2)
    m = R.Resample(48000, 16000, lowpass_filter_width=LW).to(dev)
    y64 = m.double()(x.double())                                      # float64: the torch path
    assert y64.dtype == torch.float64 and y64.shape == (3, 2334)


@pytest.mark.gpu
def test_gpu_call_allocates_only_the_output():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    m = R.Resample(44100, 16000, lowpass_filter_width=LW).to(dev)
    x = torch.randn(1, 441 * 32, device=dev)
    m(x)                                                             # builds and caches the device table
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    y = m(x)
    after = torch.cuda.memory_allocated(dev)
    assert y.numel() * 4 == 5120 * 4 and after - before == y.numel() * 4


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    k, w = R.sinc_resample_kernel(441, 160, lowpass_filter_width=6)
    bank = k[:, 0].contiguous()
    K = bank.shape[1]
    need = lib.ddsp_hip_resample_table_bytes(bank.data_ptr(), 441, 160, K)
    assert need > 0
    assert lib.ddsp_hip_resample_table_bytes(bank.data_ptr(), 441, 160, K + 1) == 0            # K - o odd
    assert lib.ddsp_hip_resample_table_bytes(bank.data_ptr(), 5000, 160, K) == 0              # o out of range
    assert lib.ddsp_hip_resample_table_bytes(None, 441, 160, K) == 0
    tab = torch.zeros(need + 64, dtype=torch.uint8)
    assert lib.ddsp_hip_resample_table(bank.data_ptr(), 441, 160, K, tab.data_ptr(), need - 1) == -4   # EWS
    assert lib.ddsp_hip_resample_table(bank.data_ptr(), 0, 160, K, tab.data_ptr(), need) == -3         # ESHAPE
    assert lib.ddsp_hip_resample_table(None, 441, 160, K, tab.data_ptr(), need) == -1                  # EINVAL
    assert lib.ddsp_hip_resample_table(bank.data_ptr(), 441, 160, K, tab.data_ptr(), need) == 0
    x = torch.randn(2, 1000)
    y = torch.zeros(2, 400)
    call = lambda **kw: lib.ddsp_hip_resample(*[kw.get(n, d) for n, d in (
        ("x", x.data_ptr()), ("ldx", 1000), ("sx", 1), ("B", 2), ("L", 1000), ("y", y.data_ptr()), ("ldy", 400),
        ("t", tab.data_ptr()), ("tb", need), ("o", 441), ("n", 160), ("w", w), ("s", None))])
    assert call() == 0
    assert call(B=0) == -1 and call(L=-1) == -1 and call(sx=-1) == -1 and call(ldx=-1) == -1 and call(w=0) == -1
    assert call(sx=0) == 0 and call(ldx=0) == 0                     # expanded inputs are legal
    assert call(o=0) == -3 and call(n=4097) == -3
    assert call(ldy=100) == -1                                       # output rows would overlap
    assert call(x=None) == -1 and call(y=None) == -1 and call(t=None) == -1
    assert call(tb=16) == -4
    assert call(t=tab.data_ptr() + 4) == -1                          # unaligned table
    assert call(L=0, x=None) == 0                                    # nothing to do
    # a table built for other rates: the kernel reads its header, no tap, and writes NaN everywhere
    y2 = torch.zeros(2, 3000)
    for o2, n2 in ((147, 160), (441, 467)):
        w2 = R.sinc_resample_kernel(o2, n2, lowpass_filter_width=6)[1]
        T2 = -(-n2 * 1000 // o2)
        y2.zero_()
        assert call(o=o2, n=n2, w=w2, y=y2.data_ptr(), ldy=3000) == 0
        assert torch.isnan(y2[:, :T2]).all() and (y2[:, T2:] == 0).all()


# ---- the reference patch hook ----------------------------------------------------------------------------------------------------

def test_patch_reference_resample(monkeypatch):
    class TAResample(torch.nn.Module):
        pass

    class Other(torch.nn.Module):
        pass

    ta = types.ModuleType("torchaudio")
    tat = types.ModuleType("torchaudio.transforms")
    tat.Resample = TAResample
    ta.transforms = tat
    monkeypatch.setitem(sys.modules, "torchaudio", ta)
    monkeypatch.setitem(sys.modules, "torchaudio.transforms", tat)
    mods = {}
    for name in ("ddsp.vocoder", "gui", "gui_diff", "enhancer", "encoder.rmvpe.inference", "diffusion.vocoder"):
        m = types.ModuleType(name)
        m.Resample = TAResample
        m.Other = Other
        monkeypatch.setitem(sys.modules, name, m)
        mods[name] = m
    mods["gui"].Resample = Other                                     # a module whose Resample is something else: untouched
    mods["enhancer"].ResampleAlias = TAResample
    early = mods["ddsp.vocoder"].Resample()
    done = R.patch_reference_resample()
    assert sorted(done) == sorted([("ddsp.vocoder", "Resample"), ("gui_diff", "Resample"), ("enhancer", "Resample"),
                                   ("enhancer", "ResampleAlias"), ("encoder.rmvpe.inference", "Resample"),
                                   ("diffusion.vocoder", "Resample")])
    for name, m in mods.items():
        assert m.Other is Other
        if name != "gui":
            assert m.Resample is R.Resample
    assert mods["gui"].Resample is Other
    assert tat.Resample is TAResample                                # torchaudio itself is left as it is
    assert type(early) is TAResample
    assert R.patch_reference_resample() == []                        # idempotent
    assert mods["ddsp.vocoder"].Resample is R.Resample


def test_patch_without_torchaudio(monkeypatch):
    monkeypatch.delitem(sys.modules, "torchaudio.transforms", raising=False)
    assert R.patch_reference_resample() == []
