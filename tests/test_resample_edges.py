"""The resampler (csrc/resample.h) at its band, phase and tile edges, bit for bit.

tests/test_resample.py holds the kernel to a float64 oracle at 1e-6.  The taps at the edge of a live band are ~1e-8 of the
result there, so a tap dropped or misplaced by the band trimming, the virtual-phase expansion or the stage / wave split passes
those bars.  Every comparison here is exact instead: the inputs make float32 arithmetic exact in any summation order, fused or
not, so a missing tap of any size fails.

  1. impulse read-out   x = a delta_p with a a power of two reads the real banks back, tap by tap: no oracle
  2. integer banks      taps in [-3, 3], samples in [-8, 8] over the phase counts n = 1 .. 97 (virtual phases, partly empty
                        tiles, several tiles), with dense, banded, one-tap, two-tap and partly all-zero banks
  3. band lengths       one tile whose band is 1 .. 257 taps long at three places: the wave predicate and the stage boundary
  4. the tap limit      a band of 65 535 taps (65 536 in the table) runs, one of 65 537 is refused
  5. dispatch           rates or bands out of range take torchaudio's op sequence (GPU only)
  6. foreign table      a table built for other rates, with virtual phases: NaN in exactly [0, T)
  7. non-finite input   where one inf / NaN sample may and must show

Synthetic banks go straight into ``R._Table``; the C entry writes into a NaN-filled buffer with ``ldy > T`` so that an output
never written or written twice over a row's end shows."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import resample_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_resample import CFG_IDS, CONFIGS, LW, _module

from ddsp_svc_amd import _ffi, resample as R  # noqa: E402

F32 = np.float32
NAN = float("nan")
HANN, KAISER = "sinc_interp_hann", "sinc_interp_kaiser"
TILE = 32                                                            # kTM, kTN and kKC of csrc/resample.h


def _table(bank, o, n, w):
    bank = np.ascontiguousarray(bank, dtype=F32)
    assert bank.shape == (n, 2 * w + o) and math.gcd(o, n) == 1
    return R._Table(torch.from_numpy(bank)[:, None], o, n, w)


def _tiles(table):
    """the table's tile headers [tiles, 4]: klo, kt (rounded up to 32), off, kl (the band as it is)"""
    words = table.host().numpy()[:32 + 16 * 128].view(np.int32)
    tiles = int(words[5])
    assert tiles == -(-O.virt_group(table.n) * table.n // TILE)
    return words[8:8 + 4 * tiles].reshape(tiles, 4)


def _abi(table, x, device, sx=1, padx=0, pady=5):
    """x [B, L] (numpy) through the C entry -> y [B, T] (numpy).  The samples lie ``sx`` apart in rows of L sx + padx floats
    whose other floats are NaN; y's rows are T + pady long and NaN-filled, and what lies behind T must still be NaN after."""
    B, L = x.shape
    T = -(-table.n * L // table.o)
    ldx, ldy = L * sx + padx, T + pady
    base = torch.full((B, ldx), NAN)
    base[:, :L * sx:sx] = torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
    base = base.to(device)
    y = torch.full((B, ldy), NAN, device=device)
    tab = table.on(device)
    _ffi.check(_ffi.lib().ddsp_hip_resample(base.data_ptr(), ldx, sx, B, L, y.data_ptr(), ldy, tab.data_ptr(), table.bytes,
                                            table.o, table.n, table.width, _ffi.stream_of(base)))
    y = y.cpu().numpy()
    assert np.isnan(y[:, T:]).all(), "wrote behind a row's end"
    return y[:, :T]


def _hip(table, x, device):
    return R.resample_hip(torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(device), table).cpu().numpy()


def _same(y, want, what):
    """bit for bit up to the sign of zero; no NaN on either side"""
    assert y.shape == want.shape and y.dtype == want.dtype == F32, (what, y.shape, want.shape)
    if not np.array_equal(y, want):
        b, t = np.argwhere(y != want)[0]
        raise AssertionError("%s: %d outputs differ, first at row %d, t = %d: got %r, want %r"
                             % (what, int((y != want).sum()), b, t, y[b, t], want[b, t]))


# ---- 1. impulse read-out of the real banks ----------------------------------------------------------------------------------------

EDGE_CONFIGS = CONFIGS + [
    (16000, 48000, LW, 0.99, HANN),                                  # n = 3: G = 10, n' = 30 (two dead lanes in the tile)
    (16000, 44100, LW, 0.99, HANN),                                  # o = 160, n = 441
    (7, 5, 6, 0.99, KAISER),                                         # n = 5: G = 6, n' = 30, no exact zero in the bank
    (3, 31, 6, 0.99, HANN),                                          # n = 31: G = 1, one dead lane
    (33, 32, 6, 0.99, HANN),                                         # n = 32: exactly one full tile
    (64, 65, 6, 0.99, HANN),                                         # n = 65: the third tile holds one phase
]
EDGE_IDS = CFG_IDS + ["%d-%d-lw%d-r%g-%s" % (a, b, lw, r, m[11:]) for a, b, lw, r, m in EDGE_CONFIGS[len(CONFIGS):]]
IMPULSE = -4.0


def _aimed(bank, o, n, w, L):
    """impulse positions that read the two end taps of every tile's band: for each tile of 32 virtual phases, the phase whose
    live band starts first and the one whose band ends last (g = 0 and g = G - 1 of the virtual copies), in the first
    output row that takes a sample at or past 0 there"""
    G = O.virt_group(n)
    live = bank != 0
    lo = np.where(live.any(1), live.argmax(1), -1)
    hi = np.where(live.any(1), bank.shape[1] - 1 - live[:, ::-1].argmax(1), -1)
    T = -(-n * L // o)
    ps = []
    for t0 in range(0, G * n, TILE):
        jv = np.arange(t0, min(t0 + TILE, G * n))
        jv = jv[lo[jv % n] >= 0]
        if not jv.size:
            continue
        first = jv[np.argmin(lo[jv % n] + (jv // n) * o)]
        last = jv[np.argmax(hi[jv % n] + (jv // n) * o)]
        for v, col in ((first, lo[first % n]), (last, hi[last % n])):
            q = v // n                                               # plain row q = q' G + g
            while col - w + q * o < 0:
                q += G
            p = int(col - w + q * o)
            assert p < L and q * n + v % n < T
            ps.append(p)
    return ps


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("cfg", EDGE_CONFIGS, ids=EDGE_IDS)
def test_impulse_reads_the_bank_back(dev, cfg):
    o, n = O.reduced(*cfg[:2])
    mod = _module(cfg)
    table, w = mod._table, mod.width
    assert table.ok
    bank = mod.kernel[:, 0].numpy()
    G = O.virt_group(n)
    edge = TILE * G * o                                              # the first sample of the second workgroup's first row
    L = edge + G * o + 7
    T = -(-n * L // o)
    spots = [0, 1, edge - 1, edge, L - 1]
    pairs = [(spots[i], spots[(i + 2) % 5]) for i in range(5)]       # B = 2, another position in each row
    for ps in pairs + [tuple(_aimed(bank, o, n, w, L))]:
        x = np.zeros((len(ps), L), F32)
        x[np.arange(len(ps)), ps] = IMPULSE
        want = np.stack([O.impulse_readout(bank, o, n, w, L, p, IMPULSE) for p in ps])
        y = _hip(table, x, dev)
        assert y.shape == (len(ps), T)
        _same(y, want, "p = %s" % (ps,))


# ---- 2. integer banks over the phase counts -----------------------------------------------------------------------------------------

NS = [1, 2, 3, 5, 7, 11, 16, 17, 31, 32, 33, 63, 64, 65, 97]
OS = [1, 3, 7, 37]
WS = [1, 5, 40, 130]
SHAPES = ["dense", "band", "impulse", "ends", "zeros"]


def _nonzero(rng, size, top=3):
    return (rng.integers(1, top + 1, size) * rng.choice([-1, 1], size)).astype(F32)


def _int_bank(shape, n, K, rng):
    if shape == "dense":
        return _nonzero(rng, (n, K))
    h = np.zeros((n, K), F32)
    if shape == "band":                                              # a live band per phase, its two end taps not zero
        for j in range(n):
            a = int(rng.integers(0, K))
            e = int(rng.integers(a, K))
            h[j, a:e + 1] = rng.integers(-3, 4, e + 1 - a)
            h[j, [a, e]] = _nonzero(rng, 2)
    elif shape == "impulse":                                         # one tap per phase
        h[np.arange(n), rng.integers(0, K, n)] = _nonzero(rng, n)
    elif shape == "ends":                                            # the first and the last tap only
        h[:, [0, K - 1]] = _nonzero(rng, (n, 2))
    else:                                                            # "zeros": all-zero phases, for n >= 64 a whole tile of them
        h = _nonzero(rng, (n, K))
        dead = rng.random(n) < 0.4
        dead[int(rng.integers(0, n))] = True
        if n >= 64:
            dead[TILE:2 * TILE] = True
        if dead.all():
            return h * 0
        h[dead] = 0
    return h


def _int_case(n, shape):
    i, s = NS.index(n), SHAPES.index(shape)
    coprime = [o for o in OS if math.gcd(o, n) == 1]
    o = coprime[(i + s) % len(coprime)]
    w = WS[(i + 2 * s + i // 4) % 4]
    return o, w


def test_integer_cases_cover_every_rate_and_width():
    picked = [_int_case(n, s) for n in NS for s in SHAPES]
    assert {o for o, _ in picked} == set(OS) and {w for _, w in picked} == set(WS)
    for s in SHAPES:
        assert len({_int_case(n, s)[1] for n in NS}) == 4, s


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_integer_banks(dev, n, shape):
    o, w = _int_case(n, shape)
    K = 2 * w + o
    G = O.virt_group(n)
    rng = np.random.default_rng(1000 * n + SHAPES.index(shape))
    bank = _int_bank(shape, n, K, rng)
    table = _table(bank, o, n, w)
    assert table.ok
    tiles = _tiles(table)
    if shape == "zeros" and n >= 64:
        assert tiles[1, 1] == 0 and tiles[1, 3] == 0 and tiles[0, 1] > 0      # an empty tile: no stage at all
    if shape == "dense":
        assert (tiles[:, 3] == (G - 1) * o + K).all() and (tiles[:, 0] == 0).all()
    edge = TILE * G * o
    # T one short of, at and one past 32 rows of outputs; the last length is past w + o, where the bank's end taps meet a sample
    for L in sorted({1, w, edge - 1, edge, edge + 1, edge + w + o}):
        if shape == "impulse":                                       # every sample another value: an index slip shows
            x = np.stack([np.arange(1, L + 1), np.arange(L, 0, -1)]).astype(F32)
        else:
            x = rng.integers(-8, 9, (2, L)).astype(F32)
        want = O.exact_apply(x, o, n, bank, w)
        _same(_abi(table, x, dev), want, "o = %d, w = %d, L = %d" % (o, w, L))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("n", [5, 33])
def test_integer_bank_strided(dev, n):
    """element stride 2 and both row strides away from their dense values; the floats between the samples are NaN"""
    o, w = 7, 5
    rng = np.random.default_rng(n)
    bank = _int_bank("band", n, 2 * w + o, rng)
    table = _table(bank, o, n, w)
    L = TILE * O.virt_group(n) * o + 1
    x = rng.integers(-8, 9, (3, L)).astype(F32)
    _same(_abi(table, x, dev, sx=2, padx=3, pady=9), O.exact_apply(x, o, n, bank, w), "strided")


# ---- 3. band lengths at the wave and stage edges ----------------------------------------------------------------------------------

LENS = [1, 31, 32, 33, 96, 97, 127, 128, 129, 160, 161, 255, 256, 257]
BAND_O, BAND_W = 3, 130
BAND_K = 2 * BAND_W + BAND_O                                        # 263
BAND_L = 2 * TILE * BAND_O + 1                                      # 65 rows of outputs, and L > w + o: every tap meets a sample


def _band_rows(rng, rows, K, a, length):
    h = np.zeros((rows, K), F32)
    h[:, a:a + length] = rng.integers(-3, 4, (rows, length))
    h[:, a] = _nonzero(rng, rows)
    h[:, a + length - 1] = _nonzero(rng, rows)
    return h


@functools.lru_cache(maxsize=None)
def _band_x():
    return _nonzero(np.random.default_rng(77), (2, BAND_L), top=8)  # no zero sample: a dropped tap changes every row it meets


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("where", ["left", "left+1", "right"])
@pytest.mark.parametrize("length", LENS)
def test_band_length_one_tile(dev, length, where):
    a = {"left": 0, "left+1": 1, "right": BAND_K - length}[where]
    rng = np.random.default_rng(10 * length + a)
    bank = _band_rows(rng, 32, BAND_K, a, length)
    table = _table(bank, BAND_O, 32, BAND_W)
    assert _tiles(table).tolist() == [[a, -(-length // TILE) * TILE, 0, length]]
    x = _band_x()
    _same(_abi(table, x, dev), O.exact_apply(x, BAND_O, 32, bank, BAND_W), "band [%d, %d)" % (a, a + length))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("length", LENS)
def test_band_length_three_tiles(dev, length):
    """n = 96: the first tile's band at the left end, the second's at the right end, the third empty"""
    rng = np.random.default_rng(length)
    o = 5                                                            # coprime to 96
    K = 2 * BAND_W + o
    bank = np.concatenate([_band_rows(rng, 32, K, 0, length), _band_rows(rng, 32, K, K - length, length),
                           np.zeros((32, K), F32)])
    table = _table(bank, o, 96, BAND_W)
    kt = -(-length // TILE) * TILE
    assert _tiles(table).tolist() == [[0, kt, 0, length], [K - length, kt, kt * TILE, length], [0, 0, 2 * kt * TILE, 0]]
    x = _nonzero(np.random.default_rng(78), (2, 2 * TILE * o + 1), top=8)
    _same(_abi(table, x, dev), O.exact_apply(x, o, 96, bank, BAND_W), "three tiles, %d taps" % length)


# ---- 4. the 65 536-tap limit ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _long_bank(K):
    return _nonzero(np.random.default_rng(K), (32, K))


def _limit_host_side(lib):
    for K, fits in ((65535, True), (65537, False)):
        bank = torch.from_numpy(_long_bank(K))
        need = lib.ddsp_hip_resample_table_bytes(bank.data_ptr(), 1, 32, K)
        if fits:                                                     # header section + 65 536 x 32 floats
            assert need == 256 + 65536 * 32 * 4
        else:
            assert need == 0
            buf = torch.zeros(1024, dtype=torch.uint8)
            assert lib.ddsp_hip_resample_table(bank.data_ptr(), 1, 32, K, buf.data_ptr(), buf.numel()) == -3
            assert not buf.any()


def test_tap_limit_host_side():
    _limit_host_side(_ffi.lib())


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_tap_limit(dev):
    _limit_host_side(_ffi.lib())
    K = 65535
    bank = _long_bank(K)
    table = _table(bank, 1, 32, K // 2)
    assert table.ok and _tiles(table).tolist() == [[0, 65536, 0, 65535]]
    x = np.random.default_rng(4).integers(-8, 9, (2, 40)).astype(F32)
    _same(_abi(table, x, dev), O.exact_apply(x, 1, 32, bank, K // 2), "K = 65535")
    refused = _table(_long_bank(65537), 1, 32, 32768)
    assert not refused.ok and refused.bytes == 0


# ---- 5. out-of-range dispatch -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("rates", [(4097, 1), (2047, 1)], ids=["o-4097", "band-past-65536"])
def test_out_of_range_takes_the_torch_path(rates, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    mod = R.Resample(*rates, lowpass_filter_width=1).to(device)
    assert mod._table is not None and not mod._table.ok and mod._table.bytes == 0
    seen = []
    orig = R._apply_torch

    def spy(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]

    def boom(*a, **k):
        raise AssertionError("entered resample_hip")
    monkeypatch.setattr(R, "_apply_torch", spy)
    monkeypatch.setattr(R, "resample_hip", boom)
    x = torch.randn(2, 3 * rates[0] + 5, device=device)
    y = mod(x)
    assert len(seen) == 1 and y is seen[0]
    assert y.shape == (2, -(-x.shape[1] // rates[0])) and y.is_cuda


# ---- 6. a table built for other rates, with virtual phases ------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("built_for", [(2, 3), (1, 2), (441, 160)], ids=lambda r: "%d-%d" % r)
def test_foreign_table_with_virtual_phases(dev, built_for):
    """the call says 1 -> 3 (G = 10, n' = 30: lanes 30 and 31 of the tile have no output)"""
    o, n, L, B, FILL = 1, 3, 331, 2, 7.0
    w = R.sinc_resample_kernel(o, n, lowpass_filter_width=6)[1]
    other = R.Resample(*built_for, lowpass_filter_width=6)._table
    assert other.ok and other.bytes >= 256 + 32
    T = n * L
    assert T % 30 and -(-T // 30) > TILE                             # a part row at the end, in a second workgroup
    x = torch.randn(B, L).to(dev)
    y = torch.full((B, T + 6), FILL, device=dev)
    tab = other.on(dev)
    assert _ffi.lib().ddsp_hip_resample(x.data_ptr(), L, 1, B, L, y.data_ptr(), T + 6, tab.data_ptr(), other.bytes, o, n, w,
                                        _ffi.stream_of(x)) == 0
    y = y.cpu()
    assert torch.isnan(y[:, :T]).all() and (y[:, T:] == FILL).all()


# ---- 7. non-finite samples --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("rates", [(3, 2, HANN), (3, 1, HANN), (7, 5, HANN), (7, 5, KAISER), (32, 33, HANN), (441, 160, HANN)],
                         ids=lambda r: "%d-%d-%s" % (r[0], r[1], r[2][11:]))
def test_one_nonfinite_sample(dev, rates):
    """Row p holds one inf, -inf or NaN, at sample p: every position of the input in one launch.  (a) an output with a non-zero
    tap on the sample is non-finite; (b) no output is outside the virtual rows whose window covers the sample (the zero taps
    that round a band up to 32 meet no sample); (c) every finite output has the bits of the run with that sample at zero."""
    o, n, method = rates
    mod = R.Resample(o, n, lowpass_filter_width=6, resampling_method=method)
    bank, w = mod.kernel[:, 0].numpy(), mod.width
    G = O.virt_group(n)
    L = 2 * G * o + 7                                                # three virtual rows of outputs, the last a part row
    p = np.arange(L)
    x0 = torch.randn(L, L, generator=torch.Generator().manual_seed(o + n)).numpy()
    x0[p, p] = 0
    x1 = x0.copy()
    x1[p, p] = np.array([np.inf, -np.inf, np.nan], F32)[p % 3]
    y0 = _hip(mod._table, x0, dev)
    y1 = _hip(mod._table, x1, dev)
    assert np.isfinite(y0).all()
    bad = ~np.isfinite(y1)
    reach = [O.reach(bank, o, n, w, L, q) for q in p]
    live, window = np.stack([r[0] for r in reach]), np.stack([r[1] for r in reach])
    assert live.any(1).all() and not window.all(1).any()
    assert bad[live].all()                                           # (a)
    assert not bad[~window].any()                                    # (b)
    assert np.array_equal(y1[~bad], y0[~bad])                        # (c)
