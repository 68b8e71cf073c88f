"""The launchers that put the utterance index on a grid's y / z axis (65 535 workgroups at most), at and past that limit.

Three of them split the batch and restart at a base utterance (csrc/resblock.h, csrc/resample.h, csrc/mel_czt.hip): the
``BATCH_SPLIT`` knob (csrc/tuning.h) lowers the chunk to 2 and 1 utterances, so that B = 5 gives chunks 2, 2, 1 -- two non-zero
bases and an uneven tail -- on the emulator and the GPU.  A split changes neither the kernel nor any per-utterance arithmetic:
the split result must EQUAL the unsplit one bit for bit, the unsplit one meets the bar of its module's own parity test against
the float64 oracle, and every utterance differs from every other (a base of zero cannot pass).  On the GPU the true limit runs
too: B = 65 537 (65 536 for the exciter), filled from a pool of 251 distinct utterances, x[b] = pool[b % 251] -- 251 is prime
and 65 535 mod 251 = 24, so a wrong base or stride moves a row onto another pool entry -- and compared bitwise with the pool's
own run, which the oracle checks.

``launch_fast_combtooth`` (csrc/stft.hip) changes kernel instead: the tests at the end reach each of its three kernels on
purpose and hold each to the float64 oracle at the bar of test_parity_fast.py (3e-7 absolute)."""
import time

import numpy as np
import pytest
import torch

from oracle import ddsp_oracle as DO
from tests import resample_oracle as SO
from tests import resblock_oracle as BO
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_mel import CFG as MEL_CFG, _check as mel_check
from tests.test_resample import _check as resample_check
from tests.test_resblock import _rms, _tensors, _torch_chain

from ddsp_svc_amd import _ffi, mel as M, nsf_generator as NG, resample as R, synth  # noqa: E402

SPLITS = (2, 1)
POOL = 251
LIMIT = 65535
SR = 44100
NAN = float("nan")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rows_differ(a):
    a = np.asarray(a)
    a = a.reshape(a.shape[0], -1)
    for i in range(a.shape[0]):
        for j in range(i + 1, a.shape[0]):
            assert not np.array_equal(a[i], a[j]), (i, j)


def _pool_index(B, device):
    return torch.arange(B, device=device) % POOL


def _timed(device, fn):
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if device.type == "cuda":
        torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def test_pool_construction():
    assert LIMIT % POOL == 24 and all(POOL % p for p in range(2, 16))


# ---- NSF-HiFiGAN ResBlock1 (csrc/resblock.h) ----------------------------------------------------------------------------------------

RB_C, RB_K = 16, 3


def _resblock_inputs(case, B, T, seed):
    """case a: one pair; case b: three pairs (both halves of the ping-pong workspace) with ``acc`` and ``scale = 3``"""
    dil = (1,) if case == "a" else (1, 3, 5)
    weights = BO.seeded_weights(RB_C, RB_K, len(dil), seed=seed)
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal((B, RB_C, T)).astype(np.float32)
    acc = None if case == "a" else rng.standard_normal((B, RB_C, T)).astype(np.float32)
    return dil, weights, x, acc, (None if case == "a" else 3)


def _resblock_reference(dil, weights, x, acc, scale):
    """the float64 oracle and test_resblock.py's bar: 4 x the float32 torch chain's own error + 1e-7 rms"""
    ref = BO.block(x, weights, dil)
    chain = torch.from_numpy(_torch_chain(x, weights, dil))
    if acc is not None:
        ref = (acc.astype(np.float64) + ref) / scale
        chain = torch.div(torch.from_numpy(acc) + chain, scale)
    return ref, 4.0 * float(np.abs(chain.numpy().astype(np.float64) - ref).max()) + 1e-7 * _rms(ref)


def _resblock_run(dil, wt, x, acc, scale):
    y = torch.full_like(x, NAN)
    assert NG.resblock1(x, wt, dil, acc=acc, scale=scale, out=y) is y
    return y


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("case", ["a", "b"])
def test_resblock_split(dev, knobs, case):
    """a: T = tile + 1, two column tiles meet the batch chunks; b: T = 7, three pairs, ``acc_in`` at a non-zero base"""
    B = 5
    T = NG.tile(RB_C, RB_K) + 1 if case == "a" else 7
    dil, weights, x, acc, scale = _resblock_inputs(case, B, T, seed=11)
    ref, bar = _resblock_reference(dil, weights, x, acc, scale)
    wt = _tensors(weights, dev)
    xt, at = torch.from_numpy(x).to(dev), None if acc is None else torch.from_numpy(acc).to(dev)
    whole = _resblock_run(dil, wt, xt, at, scale)
    assert torch.isfinite(whole).all()
    err = float(np.abs(whole.cpu().numpy().astype(np.float64) - ref).max())
    print("resblock1 case %s: error %.3e, bar %.3e" % (case, err, bar))
    assert err <= bar
    _rows_differ(whole.cpu().numpy())
    _rows_differ(ref)
    for split in SPLITS:
        knobs("BATCH_SPLIT", split)
        part = _resblock_run(dil, wt, xt, at, scale)
        assert torch.isfinite(part).all(), split
        assert torch.equal(part, whole), split


@pytest.mark.gpu
def test_resblock_past_the_grid_limit():
    """B = 65 537 = 65 535 + 2 at C = 16, k = 3, dilations (1, 3, 5), T = 3, with ``acc`` and ``scale = 3``: 12.6 MB per tensor.
    The second call must not allocate: the hand-over buffer of 2 B C T floats exists by then."""
    device = _gpu()
    B, T = LIMIT + 2, 3
    dil, weights, xp, ap, scale = _resblock_inputs("b", POOL, T, seed=21)
    ref, bar = _resblock_reference(dil, weights, xp, ap, scale)
    wt = _tensors(weights, device)
    xpool, apool = torch.from_numpy(xp).to(device), torch.from_numpy(ap).to(device)
    ypool = _resblock_run(dil, wt, xpool, apool, scale)
    assert float(np.abs(ypool.cpu().numpy().astype(np.float64) - ref).max()) <= bar
    _rows_differ(ref)
    idx = _pool_index(B, device)
    x, acc = xpool[idx].contiguous(), apool[idx].contiguous()
    y, first = _timed(device, lambda: _resblock_run(dil, wt, x, acc, scale))
    y.fill_(NAN)
    before = torch.cuda.memory_allocated(device)
    _, second = _timed(device, lambda: NG.resblock1(x, wt, dil, acc=acc, scale=scale, out=y))
    assert torch.cuda.memory_allocated(device) == before
    print("resblock1 B = %d: first call %.1f ms, second %.1f ms" % (B, 1e3 * first, 1e3 * second))
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx])


# ---- sinc resampling (csrc/resample.h) --------------------------------------------------------------------------------------------

# reduced rates: n = 2 < 32 (16 virtual phase groups in one tile) and n = 33 >= 32 (two tiles, the second holds one phase);
# lowpass_filter_width 6 keeps the bank at a few dozen taps
RS_RATES = [(3, 2), (32, 33)]
RS_L = 37


def _resample_module(o, n, device):
    return R.Resample(o, n, lowpass_filter_width=6).to(device)


def _resample_abi(mod, base, B, L, ldx, sx, ldy):
    """the C entry with every stride its own: x[b, p] = base[b ldx + p sx], y rows ``ldy`` apart in a NaN-filled buffer"""
    tab = mod._table
    dtab = tab.on(base.device)
    y = torch.full((B, ldy), NAN, device=base.device)
    _ffi.check(_ffi.lib().ddsp_hip_resample(base.data_ptr(), ldx, sx, B, L, y.data_ptr(), ldy, dtab.data_ptr(), tab.bytes, tab.o,
                                            tab.n, tab.width, _ffi.stream_of(base)))
    return y


def _resample_layout(layout, device):
    """-> (x as the caller sees it [.., L], run(x) -> y of x's leading shape)"""
    g = torch.Generator().manual_seed(len(layout) + 3)
    L = RS_L
    if layout == "dense":
        x = torch.randn(5, L, generator=g).to(device)
    elif layout == "rows":                                           # a row view: stride(0) > L
        x = torch.randn(5, L + 7, generator=g).to(device)[:, :L]
        assert x.stride(0) > L and not x.is_contiguous()
    elif layout == "3d":                                             # [2, 3, L] flattened to 6 rows
        x = torch.randn(2, 3, L, generator=g).to(device)
    else:                                                            # "abi": ldx, sx and ldy all away from the dense values
        base = torch.randn(5, 2 * L + 5, generator=g).to(device)
        x = base[:, :2 * L:2]
        assert x.stride() == (2 * L + 5, 2)

        def run(mod):
            T = -(-mod._table.n * L // mod._table.o)
            y = _resample_abi(mod, base, 5, L, 2 * L + 5, 2, T + 3)
            assert torch.isnan(y[:, T:]).all()                       # nothing behind a row's end
            return y[:, :T]
        return x, run
    return x, lambda mod: R.resample_hip(x, mod._table)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("layout", ["dense", "rows", "3d", "abi"])
@pytest.mark.parametrize("rates", RS_RATES, ids=lambda r: "%d-%d" % r)
def test_resample_split(dev, knobs, rates, layout):
    o, n = rates
    mod = _resample_module(o, n, dev)
    assert (mod._table.n < 32) == (n < 32) and mod._table.ok
    x, run = _resample_layout(layout, dev)
    whole = run(mod)
    assert whole.shape == x.shape[:-1] + (-(-n * RS_L // o),)
    assert torch.isfinite(whole).all()
    ref = SO.apply(x.cpu().numpy(), o, n, mod.kernel[:, 0].cpu().numpy(), mod.width)
    resample_check(whole, ref, x, layout)
    _rows_differ(whole.reshape(-1, whole.shape[-1]).cpu().numpy())
    _rows_differ(ref.reshape(-1, ref.shape[-1]))
    for split in SPLITS:
        knobs("BATCH_SPLIT", split)
        part = run(mod)
        assert torch.isfinite(part).all(), split
        assert torch.equal(part, whole), split


@pytest.mark.gpu
def test_resample_past_the_grid_limit():
    """B = 65 537 rows of L = 16 samples at 3 -> 2 (11 output samples each), through the strided C entry: 4 MB in, 3 MB out"""
    device = _gpu()
    o, n = RS_RATES[0]
    B, L = LIMIT + 2, 16
    mod = _resample_module(o, n, device)
    T = -(-n * L // o)
    pool = torch.randn(POOL, L, generator=torch.Generator().manual_seed(5)).to(device)
    ypool = R.resample_hip(pool, mod._table)
    ref = SO.apply(pool.cpu().numpy(), o, n, mod.kernel[:, 0].cpu().numpy(), mod.width)
    resample_check(ypool, ref, pool)
    _rows_differ(ref)
    idx = _pool_index(B, device)
    x = pool[idx].contiguous()
    y, took = _timed(device, lambda: R.resample_hip(x, mod._table))
    print("resample B = %d: %.1f ms" % (B, 1e3 * took))
    assert y.shape == (B, T) and torch.equal(y, ypool[idx])
    base = torch.zeros(B, L + 3, device=device)                      # and with ldx, ldy away from L, T
    base[:, :L] = x
    ys = _resample_abi(mod, base, B, L, L + 3, 1, T + 5)
    assert torch.isnan(ys[:, T:]).all() and torch.equal(ys[:, :T], ypool[idx])


# ---- the log-mel front-end's chirp-z path (csrc/mel_czt.hip) ------------------------------------------------------------------------

MEL_SHIFTS = {-12: 4, 3: 8}                                          # key shift -> the k_mel_czt<R> it selects at n_fft = 2048


def _mel_pad_right(T, win, hop):
    return max((win - hop + 1) // 2, win - T - (win - hop) // 2)     # nvSTFT.py:97-103


def _mel_reflects(T, win, hop):
    return _mel_pad_right(T, win, hop) < T


def _mel_shortest_reflecting(win, hop):
    return next(T for T in range(1, 4 * win) if _mel_reflects(T, win, hop))


def _mel_audio(B, T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T) / float(SR)
    b = np.arange(B)[:, None]
    return ((0.2 + 0.05 * (b % 7)) * np.sin(2 * np.pi * (220.0 + 3.0 * b) * t[None]) + 0.1 * rng.standard_normal((B, T))).astype(np.float32)


class _MelShifted:
    """``STFT.get_mel(y, keyshift)`` through the C entry into a NaN-filled store whose utterances lie ``frames n_mels + pad``
    floats apart (mel.py only ever passes the dense stride)"""

    def __init__(self, keyshift, device, pad=5):
        self.stft = M.STFT(**MEL_CFG)
        _, (self.band, self.packed), _ = self.stft._tables(device)
        self.n_new, self.win_new, self.hop_new = M._shifted_sizes(2048, 2048, 512, keyshift, 1)
        self.n_bins = 1025
        self.scale = 2048 / self.win_new
        self.tab = M.shifted_tables(self.n_new, self.win_new, self.n_bins, device)
        self.pad, self.keyshift = pad, keyshift
        lib = _ffi.lib()
        assert lib.ddsp_hip_mel_shifted_table_bytes(self.n_new, self.n_bins) == 8 * (
            512 * MEL_SHIFTS[keyshift] + (256 * MEL_SHIFTS[keyshift] + 128 * MEL_SHIFTS[keyshift] + 1) * 2 *
            ((-(-self.n_new // (256 * MEL_SHIFTS[keyshift])) + 1) // 2))      # the table of the plan R: pins which kernel runs

    def __call__(self, audio):
        lib = _ffi.lib()
        B, T = audio.shape
        frames = lib.ddsp_hip_mel_shifted_frames(T, self.n_new, self.win_new, self.hop_new, 0)
        assert frames >= 1
        n = frames * 128
        store = torch.full((B, n + self.pad), NAN, device=audio.device)
        _ffi.check(lib.ddsp_hip_mel_shifted_spectrogram(audio.data_ptr(), B, T, self.tab.data_ptr(), self.n_new, self.win_new,
                                                        self.hop_new, 0, self.n_bins, float(self.scale), self.band.data_ptr(),
                                                        self.packed.data_ptr(), 128, 1e-5, store.data_ptr(), n + self.pad, 1, 128,
                                                        _ffi.stream_of(audio)))
        assert torch.isnan(store[:, n:]).all()
        return store[:, :n].view(B, frames, 128).transpose(1, 2)


def _mel_reference(audio, keyshift):
    return DO.get_mel(audio, DO.mel_filterbank_slaney(SR, 2048, 128, 40, 16000), keyshift=keyshift)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zeros"])
@pytest.mark.parametrize("keyshift", sorted(MEL_SHIFTS))
def test_mel_shifted_split(dev, knobs, keyshift, reflect):
    run = _MelShifted(keyshift, dev)
    T = _mel_shortest_reflecting(run.win_new, run.hop_new) if reflect else 100
    assert _mel_reflects(T, run.win_new, run.hop_new) == reflect and not _mel_reflects(T - 1, run.win_new, run.hop_new)
    audio = _mel_audio(5, T, seed=T)
    at = torch.from_numpy(audio).to(dev)
    whole = run(at)
    assert torch.isfinite(whole).all()
    ref = _mel_reference(audio, keyshift)
    assert whole.shape == ref.shape
    mel_check(whole.cpu().numpy(), ref)
    _rows_differ(whole.cpu().numpy())
    _rows_differ(ref)
    for split in SPLITS:
        knobs("BATCH_SPLIT", split)
        part = run(at)
        assert torch.isfinite(part).all(), split
        assert torch.equal(part, whole), split


@pytest.mark.gpu
def test_mel_shifted_past_the_grid_limit():
    """B = 65 537 utterances of one hop (512 samples, one frame each) at key shift -12 (k_mel_czt<4>): 134 MB of audio, 34 MB out"""
    device = _gpu()
    B, T = LIMIT + 2, 512
    run = _MelShifted(-12, device)
    audio = _mel_audio(POOL, T, seed=9)
    pool = torch.from_numpy(audio).to(device)
    ypool = run(pool)
    ref = _mel_reference(audio, -12)
    mel_check(ypool.cpu().numpy(), ref)
    _rows_differ(ref)
    idx = _pool_index(B, device)
    x = pool[idx].contiguous()
    y, took = _timed(device, lambda: run(x))
    print("mel chirp-z B = %d: %.1f ms" % (B, 1e3 * took))
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx])


# ---- the three exciter kernels of launch_fast_combtooth (csrc/stft.hip) ----------------------------------------------------------------

COMB_BAR = 3e-7                                                      # test_parity_fast.py: float32 sine and divide inside sinc


def _comb_f0(B, F, hop, seed):
    f0 = DO.synth_f0(B, F, SR, hop, seed=seed)[:, :, 0].copy()
    if F > 2:
        f0[0, 1] = 0.0                                               # an unvoiced frame
        f0[1, 2] = min(2.2 * f0[1, 1], 800.0)                        # a jump from one frame to the next
        f0[2, 0] = 0.0
    return f0


def _comb_entry(f0, hop):
    """through ``synth.fast_source``: its output is an allocation of its own, 16-byte aligned"""
    st = synth.fast_source(f0, SR, hop, want_combtooth=True)
    assert st.combtooth.data_ptr() % 16 == 0
    return st.combtooth


def _comb_abi(f0, hop, offset):
    """through the C entry into a view ``offset`` floats behind a 16-byte boundary of a NaN-filled buffer"""
    B, F = f0.shape
    n = B * F * hop
    rad, pf = torch.empty(B, F, device=f0.device), torch.empty(B, F, 1, device=f0.device)
    buf = torch.full((n + 8,), NAN, device=f0.device)
    assert buf.data_ptr() % 16 == 0
    comb = buf[offset:offset + n]
    _ffi.check(_ffi.lib().ddsp_hip_fast_source(f0.data_ptr(), B, F, hop, float(SR), rad.data_ptr(), pf.data_ptr(), comb.data_ptr(),
                                               _ffi.stream_of(f0)))
    assert torch.isnan(buf[:offset]).all() and torch.isnan(buf[offset + n:]).all()
    return comb.view(B, F * hop)


COMB_KERNELS = {
    "vector-pow2": (512, lambda f0: _comb_entry(f0, 512)),           # k_fast_combtooth4<true>
    "vector-div": (12, lambda f0: _comb_entry(f0, 12)),              # k_fast_combtooth4<false>
    "scalar-hop441": (441, lambda f0: _comb_entry(f0, 441)),         # k_fast_combtooth: hop % 4 != 0
    "scalar-misaligned": (512, lambda f0: _comb_abi(f0, 512, 1)),    # k_fast_combtooth: out one float off a 16-byte boundary
}


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("kernel", sorted(COMB_KERNELS))
def test_fast_combtooth_kernels(dev, kernel):
    hop, run = COMB_KERNELS[kernel]
    f0 = _comb_f0(3, 5, hop, seed=hop)
    comb = run(torch.from_numpy(f0).to(dev))
    ref, _, _ = DO.fast_source_gen(f0, SR, hop)
    assert comb.shape == ref.shape and torch.isfinite(comb).all()
    err = float(np.abs(comb.cpu().numpy().astype(np.float64) - ref).max())
    print("%s: error %.3e" % (kernel, err))
    assert err <= COMB_BAR
    _rows_differ(ref)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_fast_combtooth_scalar_against_vector(dev):
    """hop 512, aligned (k_fast_combtooth4<true>) against misaligned (k_fast_combtooth): each is within one bar of the same
    oracle, so they are within two of each other"""
    f0 = torch.from_numpy(_comb_f0(3, 5, 512, seed=512)).to(dev)
    vec, sca = _comb_entry(f0, 512), _comb_abi(f0, 512, 1)
    diff = float((vec - sca).abs().max())
    print("scalar against vector exciter at hop 512: %.3e" % diff)
    assert diff <= 2 * COMB_BAR


@pytest.mark.gpu
def test_fast_combtooth_past_the_grid_limit():
    """B = 65 536, F = 2, hop 512 through ``synth.fast_source``: past the vector kernels' grid, so the scalar kernel -- the same
    bits as the pool's rows from the scalar kernel (forced there by a misaligned output).  268 MB of samples."""
    device = _gpu()
    B, F, hop = LIMIT + 1, 2, 512
    f0p = DO.synth_f0(POOL, F, SR, hop, seed=3)[:, :, 0].copy()
    f0p[7] = 0.0
    f0p[11, 1] = 0.0
    pool = torch.from_numpy(f0p).to(device)
    cpool = _comb_abi(pool, hop, 1)
    ref, _, _ = DO.fast_source_gen(f0p, SR, hop)
    assert float(np.abs(cpool.cpu().numpy().astype(np.float64) - ref).max()) <= COMB_BAR
    idx = _pool_index(B, device)
    f0 = pool[idx].contiguous()
    comb, took = _timed(device, lambda: _comb_entry(f0, hop))
    print("fast exciter B = %d: %.1f ms" % (B, 1e3 * took))
    assert comb.shape == (B, F * hop)
    for lo in range(0, B, 16384):                                    # in slices: the gathered pool rows are 268 MB otherwise
        assert torch.equal(comb[lo:lo + 16384], cpool[idx[lo:lo + 16384]]), lo
