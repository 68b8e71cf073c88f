"""The frame features of the real-time path (ddsp_svc_amd.features, csrc/frame_features.h) against the float64 oracle
(tests/features_oracle.py), which is itself pinned to the reference's own results (tests/golden/features_*.npz,
make_golden_features.py).  Every comparison that decides a result is tested AT its boundary: a flip fails, nothing is excluded."""
import sys
import types

import numpy as np
import pytest
import torch

from tests import features_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401

EINVAL, ESHAPE, EWS = -1, -3, -4
SR = 44100


def _load(golden_dir, name):
    return np.load("%s/%s.npz" % (golden_dir, name))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30))) if want.size else 0.0


def _assert_track(got, want, ulps=2):
    """within ``ulps`` float32 ulp of the oracle, zeros (the unvoiced pattern) equal"""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0)
    u = O.ulp_diff(got, want)
    assert u.max() <= ulps, (int(np.argmax(u)), u.max())


# ---- the oracle against the reference's own results (no library) -------------------------------------------------------------
def test_oracle_reproduces_reference_volume(golden_dir):
    z = _load(golden_dir, "features_volume")
    for hop in (160, 512):
        got, want = O.volume(z["audio_%d" % hop], hop), z["volume_%d" % hop]
        assert want.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got == 0, want == 0) and np.any(want == 0)
        assert _rel(got[want != 0], want[want != 0]) <= 2e-6


def test_oracle_reproduces_reference_infer(golden_dir):
    """the whole of SvcDDSP.infer: the mask it multiplied into a model output of ones, and the f0 and volume it gave the model"""
    z = _load(golden_dir, "features_infer")
    block, sr, db, start, f0_min = (int(v) for v in z["sizes"])
    vol = O.volume(z["audio"], block)
    assert _rel(vol, z["volume"]) <= 2e-6
    assert O.volume_margin(vol, db) > 1e-5                          # float32 and float64 volumes threshold alike
    fm = O.frame_mask(z["volume"], db)
    assert np.array_equal(fm, O.frame_mask(vol.astype(np.float32), db)) and 0 < fm.sum() < fm.size
    assert np.array_equal(O.upsample_torch_f32(fm, block), z["mask"])                  # torch's float32 interpolation, bit for bit
    assert np.max(np.abs(O.upsample(fm, block) - z["mask"])) <= 2e-7                   # the exact ramp: float32(scale i) rounds
    n = vol.shape[0]
    want = O.f0_track(z["f0_src"], 0.01, block, sr, n, start, "linear", True, float(f0_min))
    _assert_track(z["f0"], want)


def test_oracle_reproduces_reference_decode(golden_dir):
    z = _load(golden_dir, "features_decode")
    for got, want in ((O.decode_salience(z["hidden"])[0], z["f0"]),
                      (O.decode_salience(z["hidden"], center=z["center"])[0], z["f0_center"])):
        assert np.array_equal(got == 0, want == 0) and np.any(want == 0) and np.any(want != 0)
        assert _rel(got[want != 0], want[want != 0]) <= 2e-6
    assert np.argmax(z["hidden"][0, 12]) == 100 and z["hidden"][0, 12, 200] == z["hidden"][0, 12, 100]      # the tie


def test_oracle_reproduces_reference_track(golden_dir):
    z = _load(golden_dir, "features_track")
    hop, sr, n, start = (int(v) for v in z["rmvpe_sizes"])
    for uv in (0, 1):
        _assert_track(z["rmvpe_uv%d" % uv], O.f0_track(z["rmvpe_src"], 0.01, hop, sr, n, 0, "linear", bool(uv)))
        _assert_track(z["rmvpe_front_uv%d" % uv], O.f0_track(z["rmvpe_src"], 0.01, hop, sr, n, start, "linear", bool(uv)))
        _assert_track(z["crepe_front_uv%d" % uv], O.f0_track(z["crepe_pooled"][0], 0.005, hop, sr, n, start, "nearest", bool(uv)))
    assert start > 0 and np.any(z["rmvpe_front_uv0"] == 0) and not np.any(z["rmvpe_front_uv1"] == 0)


def test_oracle_reproduces_reference_pools(golden_dir):
    z = _load(golden_dir, "features_pools")
    for k in (3, 4, 9):
        assert _rel(O.masked_avg_pool(z["x"], k), z["avg_%d" % k]) <= 1e-6
        assert np.array_equal(O.median_pool(z["x"], k), z["median_%d" % k], equal_nan=True)
    assert np.any(z["avg_9"] == 0) and np.any(np.isnan(z["median_3"]))
    # the crepe branch's own chain (features_track.npz): MedianPool1d, the threshold, MaskedAvgPool1d
    t = _load(golden_dir, "features_track")
    f0 = t["crepe_raw"].copy()
    f0[O.median_pool(t["crepe_pd"], 4) < np.float32(0.05)] = np.nan
    assert _rel(O.masked_avg_pool(f0, 4), t["crepe_pooled"]) <= 1e-6


# ---- volume -------------------------------------------------------------------------------------------------------------------
def _audio(B, T, seed):
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.uniform(0.0, 1.0, (B, T // 64 + 1)), 64, axis=1)[:, :T] ** 2
    return (env * rng.standard_normal((B, T))).astype(np.float32)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("hop,T,B", [(160, 160 * 9, 1), (160, 160 * 9 + 81, 5), (441, 441 * 6, 5), (441, 441 * 5 + 220, 1),
                                     (512, 512 * 6, 5), (512, 512 * 5 + 257, 1), (2048, 2048 * 3, 1), (2048, 2048 * 2 + 1025, 5),
                                     (512, 300, 1), (3, 8, 2)])
def test_volume_against_oracle(dev, hop, T, B):
    from ddsp_svc_amd import features
    a = _audio(B, T, hop + T)
    a[:, hop: min(3 * hop, T)] = 0                                  # frames that hold nothing but zeros
    want = O.volume(a, hop)
    got = features.volume(_t(a, dev), hop).cpu().numpy()
    assert got.shape == (B, T // hop + 1) and got.dtype == np.float32
    assert O.ulp_diff(got, want).max() <= 1
    assert np.array_equal(got == 0, want == 0) and (T < 3 * hop or np.any(got == 0))
    one = features.volume(_t(a[0], dev), float(hop)).cpu().numpy()  # a [T] input, an integral float hop
    assert one.shape == (T // hop + 1,) and np.array_equal(one, got[0])
    off = torch.zeros(B, T + 3, dtype=torch.float32, device=dev)    # rows that start off the 16-byte grid: the same bits
    off[:, 3:] = _t(a, dev)
    assert np.array_equal(features.volume(off[:, 3:], hop).cpu().numpy(), got)


# ---- mask and gate ------------------------------------------------------------------------------------------------------------
def _check_gate(dev, vol, db, block, dilate=4, seed=0):
    from ddsp_svc_amd import features
    vol = np.atleast_2d(np.asarray(vol, np.float32))
    B, F = vol.shape
    fm = O.frame_mask(vol, db, dilate)
    got_fm = features.silence_mask(_t(vol, dev), db, dilate=dilate).cpu().numpy()
    assert np.array_equal(got_fm, fm.astype(np.float32))
    sig = np.random.default_rng(seed).standard_normal((B, F * block)).astype(np.float32)
    up = O.upsample(fm, block)
    want = sig.astype(np.float64) * up
    out = features.gate(_t(sig, dev), _t(vol, dev), db, block, dilate).cpu().numpy()
    assert O.ulp_diff(out, want).max() <= 1
    flat = (up == 0) | (up == 1)
    assert np.array_equal(out[flat], (sig * up.astype(np.float32))[flat])                  # exact where the mask is 0 or 1
    s = _t(sig.copy(), dev)                                         # (on the emu leg the tensor IS the array)
    assert features.gate(s, _t(vol, dev), db, block, dilate, out=s) is s and np.array_equal(s.cpu().numpy(), out)   # in place
    up_got = features.silence_mask(_t(vol, dev), db, block, dilate).cpu().numpy()
    assert O.ulp_diff(up_got, up).max() <= 1 and np.array_equal(up_got[flat], up.astype(np.float32)[flat])
    if B == 1:
        assert np.array_equal(features.gate(_t(sig[0], dev), _t(vol[0], dev), db, block, dilate).cpu().numpy(), out[0])
    return fm


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B,F,block,hop", [(1, 40, 512, 512), (3, 23, 441, 160), (2, 11, 37, 2048), (1, 30, 3, 441)])
def test_gate_against_oracle(dev, B, F, block, hop):
    rng = np.random.default_rng(F)
    T = hop * (F - 1) + hop // 3
    loud = np.zeros((B, F + 1), bool)
    for b in range(B):                                              # one loud stretch per row, a second where the row has room
        loud[b, (7 * b + 1) % F] = True
        loud[b, (7 * b + 16) % F: (7 * b + 16) % F + 2] = F >= 30
    env = np.repeat(np.where(loud, 0.1, 1e-4), hop, axis=1)[:, :T]
    audio = (env * rng.standard_normal((B, T))).astype(np.float32)
    vol = O.volume(audio, hop)
    assert vol.shape == (B, F) and O.volume_margin(vol, -45) > 1e-5             # asserted on the oracle, nothing excluded
    fm = _check_gate(dev, vol.astype(np.float32), -45, block)
    assert 0 < fm.sum() < fm.size


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_gate_threshold_and_dilation_edges(dev):
    thr = O.threshold(-45)
    above = np.nextafter(thr, np.float32(1))
    for F in (30, 9, 8, 5, 1):                                      # F < 9: the window is wider than the row
        for pos in sorted({0, F - 1, F // 2}):
            for loud, n_on in ((above, min(F, pos + 5) - max(0, pos - 4)), (thr, 0)):    # equal to the threshold: mask 0
                vol = np.full(F, 1e-5, np.float32)
                vol[pos] = loud
                fm = _check_gate(dev, vol, -45, 16, seed=F + pos)
                assert fm.sum() == n_on, (F, pos, float(loud))
    vol = np.full((2, 12), 1e-5, np.float32)
    vol[0, 0] = vol[1, 11] = 1.0
    for d, n_on in ((0, 1), (1, 2), (11, 12)):
        assert _check_gate(dev, vol, -45, 8, dilate=d).sum() == 2 * n_on


# ---- decode -------------------------------------------------------------------------------------------------------------------
def _salience(B, N, seed, peaks=None):
    rng = np.random.default_rng(seed)
    h = (rng.uniform(0, 0.02, (B, N, 360)) ** 2).astype(np.float32)
    c = rng.integers(5, 355, (B, N)) if peaks is None else np.asarray(peaks).reshape(B, N)
    for b in range(B):
        for i in range(N):
            w = np.exp(-0.5 * ((np.arange(360) - c[b, i] - rng.uniform(-0.4, 0.4)) / 1.3) ** 2)
            h[b, i] += (rng.uniform(0.2, 0.9) * w).astype(np.float32)
    return h


def _check_decode(dev, h, thred=0.03, center=None):
    from ddsp_svc_amd import features
    want = O.decode_salience(h, thred, center)
    got = features.decode_salience(_t(h, dev), thred, None if center is None else _t(center, dev)).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got == 0, want == 0)
    assert _rel(got[want != 0], want[want != 0]) <= 1e-6
    return got


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_decode_against_oracle(dev):
    h = _salience(2, 9, 1)
    h[1, 3] = 0                                                     # an all-zero row
    h[1, 4] *= np.float32(0.01)
    got = _check_decode(dev, h)
    assert got[1, 3] == 0 and got[1, 4] == 0 and np.count_nonzero(got) == 16
    edge = _salience(1, 4, 2, peaks=[0, 3, 356, 359])               # the clipped windows
    assert [int(np.argmax(r)) for r in edge[0]] == [0, 3, 356, 359]
    _check_decode(dev, edge)
    rng = np.random.default_rng(3)
    c = rng.integers(0, 360, (2, 9))
    c[0, :4] = (0, 2, 357, 359)
    _check_decode(dev, h, center=c)
    from ddsp_svc_amd import features
    got3 = features.decode_salience(_t(h, dev), center=_t(c[..., None], dev)).cpu().numpy()       # the reference's [B, T, 1]
    assert np.array_equal(got3, features.decode_salience(_t(h, dev), center=_t(c, dev)).cpu().numpy())


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_decode_ties_and_threshold_boundary(dev):
    h = _salience(1, 6, 4)
    top = h[0].max() + np.float32(0.25)
    h[0, 0, [310, 40, 170]] = top                                   # a tie across lanes: bin 40
    h[0, 1, [65, 64]] = top                                         # neighbours across the lane wrap: bin 64
    h[0, 2, [359, 0]] = top
    assert [int(np.argmax(h[0, i])) for i in range(3)] == [40, 64, 0]
    got = _check_decode(dev, h)
    lone = np.zeros((1, 3, 360), np.float32)                        # one bin each: f0 is that bin's pitch exactly
    lone[0, 0, [310, 40, 170]] = 1                                  # ... the window of the FIRST of the tied bins
    lone[0, 1, 64] = lone[0, 1, 300] = 1
    lone[0, 2, 359] = lone[0, 2, 0] = 1
    got = _check_decode(dev, lone)
    for i, c in enumerate((40, 64, 0)):
        assert abs(got[0, i] / (10 * 2 ** ((20 * c + O.CENTS_BASE) / 1200)) - 1) <= 1e-6
    thr = np.float32(0.03)
    b = _salience(1, 2, 5)
    b[0] *= thr / b[0].max(axis=1, keepdims=True)
    b[0, 0, np.argmax(b[0, 0])] = thr                               # a maximum equal to float32(0.03): voiced
    b[0, 1, np.argmax(b[0, 1])] = thr
    b[0, 1][b[0, 1] >= thr] = np.nextafter(thr, np.float32(0))      # one float32 below: unvoiced
    assert b[0, 0].max() == thr and b[0, 1].max() == np.nextafter(thr, np.float32(0))
    got = _check_decode(dev, b)
    assert got[0, 0] > 0 and got[0, 1] == 0


# ---- track --------------------------------------------------------------------------------------------------------------------
def _src(n, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    f0 = (200.0 + 80.0 * np.sin(np.arange(n) / 6.0 + rng.uniform(0, 6)) + rng.uniform(-4, 4, n)).astype(np.float32)
    if kind == "voiced":
        return f0
    if kind == "unvoiced":
        return np.zeros(n, np.float32)
    if kind == "single":
        out = np.zeros(n, np.float32)
        out[n // 3] = f0[n // 3]
        return out
    f0[: 1 + n // 20] = 0                                           # unvoiced at both ends
    f0[n - 2 - n // 25:] = 0
    for _ in range(max(1, n // 12)):
        s = int(rng.integers(2, n - 3))
        f0[s: s + int(rng.integers(1, 7))] = 0
    return f0


def _check_track(dev, rows, period, hop, sr, n, start=0, mode="linear", uv=False, f0_min=65.0):
    from ddsp_svc_amd import features
    rows = np.atleast_2d(rows)
    if mode == "linear":                                            # asserted on the oracle, nothing excluded
        for r in rows if n > start else ():
            assert np.min(np.abs(O.retimed_uv(r, period, hop, sr, n - start) - 0.5)) >= 1e-6
    want = np.stack([O.f0_track(r, period, hop, sr, n, start, mode, uv, f0_min) for r in rows])
    got = features.f0_track(_t(rows, dev), period, hop, sr, n, start, mode, uv, f0_min).cpu().numpy()
    _assert_track(got, want)
    if rows.shape[0] == 1:
        one = features.f0_track(_t(rows[0], dev), period, hop, sr, n, start, mode, uv, f0_min).cpu().numpy()
        assert np.array_equal(one, got[0])
    return got


GRIDS = [(512, 44100, 0.01), (256, 44100, 0.01), (160, 16000, 0.01), (480, 48000, 0.01)]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("hop,sr,period", GRIDS)
@pytest.mark.parametrize("uv", [False, True])
def test_track_linear_against_oracle(dev, hop, sr, period, uv):
    N = 150
    n = int(N * period * sr / hop) + 12                             # longer than the source covers: the end value is held
    rows = np.stack([_src(N, 1), _src(N, 2), _src(N, 3, "voiced"), _src(N, 4, "unvoiced"), _src(N, 5, "single")])
    got = _check_track(dev, rows, period, hop, sr, n, 0, "linear", uv, 65.0)
    assert np.all(got[3] == (65.0 if uv else 0.0))                  # all unvoiced: zeros, or all f0_min
    assert not np.any(got[2] == 0) and (uv or np.any(got[0] == 0))
    if uv:
        assert not np.any(got == 0) and got.min() >= 65.0
    _check_track(dev, rows, period, hop, sr, n, 7, "linear", uv, 250.0)                   # a prefix, a floor that bites
    _check_track(dev, rows[:1], period, hop, sr, 5, 5, "linear", uv)                      # nothing but the prefix
    _check_track(dev, rows[:1, :1], period, hop, sr, 4, 1, "linear", uv)                  # N = 1


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("uv", [False, True])
def test_track_nearest_against_oracle(dev, uv):
    rows = np.stack([_src(260, 6), _src(260, 7, "unvoiced"), _src(260, 8, "single")])
    for hop, sr in ((512, 44100), (441, 44100), (160, 16000)):      # 441 / 44100 / 0.005 = 2 k; 160 / 16000: ties at k + 0.5
        _check_track(dev, rows, 0.005, hop, sr, int(260 * 0.005 * sr / hop) + 9, 3, "nearest", uv)
    half = np.arange(1, 41, dtype=np.float32)                       # 2.5 source steps per frame: round half to even
    assert [int(np.round(k * 200 / 16000 / 0.005)) for k in range(5)] == [0, 2, 5, 8, 10]
    got = _check_track(dev, half, 0.005, 200, 16000, 12, 0, "nearest", uv)
    assert got[0, :5].tolist() == ([65.0] * 5 if uv else [1.0, 3.0, 6.0, 9.0, 11.0])


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_track_spans_several_chunks(dev):
    """N and n_frames past the workgroup's 1024-element chunk: the carries of both scans"""
    N = 2300
    f0 = _src(N, 9)
    f0[900:1200] = 0                                                # an unvoiced stretch across a chunk edge
    f0[2040:2060] = 0
    _check_track(dev, f0, 0.01, 256, 44100, int(N * 0.01 * 44100 / 256) + 3, 2, "linear", True)
    lone = np.zeros(N, np.float32)
    lone[2100] = 123.0                                              # one voiced frame in the last chunk feeds the first
    _check_track(dev, lone, 0.01, 512, 44100, 2070, 0, "linear", True)


@pytest.mark.gpu
def test_track_of_a_ten_minute_file():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N = 70000
    f0 = _src(N, 10)
    _check_track(torch.device("cuda:0"), f0, 0.01, 512, 44100, int(N * 0.01 * 44100 / 512) + 1, 0, "linear", True)


# ---- pools --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 9, 16])
def test_pools_against_oracle(dev, k):
    from ddsp_svc_amd import core
    rng = np.random.default_rng(k)
    x = rng.uniform(50, 400, (3, 301)).astype(np.float32)
    x[0, rng.integers(0, 301, 60)] = np.nan
    x[1, 100:140] = np.nan                                          # windows that hold nothing but NaN
    x[2, [0, 300]] = np.nan
    x[2, 50:60] = x[2, 50]                                          # equal values
    avg = core.MaskedAvgPool1d(_t(x, dev), k).cpu().numpy()
    want = O.masked_avg_pool(x, k)
    assert avg.shape == x.shape and not np.any(np.isnan(avg)) and np.array_equal(avg == 0, want == 0)
    assert _rel(avg, want) <= 1e-6 and np.all(avg[1, 108:132] == 0)
    med = core.MedianPool1d(_t(x, dev), k).cpu().numpy()
    assert np.array_equal(med, O.median_pool(x, k), equal_nan=True)
    if k == 1:
        assert np.array_equal(med, x, equal_nan=True) and np.array_equal(avg, np.nan_to_num(x))
    short = x[:, : k // 2 + 1]                                      # the shortest row the reflection allows
    assert np.array_equal(core.MedianPool1d(_t(short, dev), k).cpu().numpy(), O.median_pool(short, k), equal_nan=True)
    assert _rel(core.MaskedAvgPool1d(_t(short, dev), k).cpu().numpy(), O.masked_avg_pool(short, k)) <= 1e-6


# ---- the session --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B", [1, 2])
def test_streaming_features_match_the_functional_forms(dev, B):
    from ddsp_svc_amd import features
    hop, block, T, N = 160, 96, 160 * 30 + 50, 40
    sess = features.StreamingFeatures(B, T, hop, N, 0.01, 16000, block, -45, dilate=4, start_frame=2, uv_interp=True, f0_min=70.0,
                                      device=dev)
    F = T // hop + 1
    blocks = []
    for i in range(3):
        rng = np.random.default_rng(50 + i)
        env = np.repeat(np.where(rng.uniform(size=(B, F + 1)) < 0.06, 0.1, 1e-4), hop, axis=1)[:, :T]
        a = _t((env * rng.standard_normal((B, T))).astype(np.float32), dev)
        f = _t(np.stack([_src(N, 60 + 7 * i + b) for b in range(B)]), dev)
        s = _t(rng.standard_normal((B, F * block)).astype(np.float32), dev)
        blocks.append((a[0], f[0], s[0]) if B == 1 else (a, f, s))
    for a, f, s in blocks:                                          # warm: the library, the allocator
        features.gate(s, features.volume(a, hop), -45, block)
    outs = []
    for a, f, s in blocks:
        s2 = s.clone()                                              # the caller's, made before the step
        before = torch.cuda.memory_allocated() if dev.type == "cuda" else 0
        v = sess.volume(a)
        t = sess.track(f)
        g = sess.gate_(s2)
        if dev.type == "cuda":
            assert torch.cuda.memory_allocated() == before          # no allocation after construction
        assert g is s2
        outs.append((v.clone(), t.clone(), g))
    for (a, f, s), (v, t, g) in zip(blocks, outs):
        wv = features.volume(a, hop)
        assert v.shape == wv.shape and torch.equal(v, wv)
        assert torch.equal(t, features.f0_track(f, 0.01, hop, 16000, F, 2, "linear", True, 70.0))
        assert torch.equal(g, features.gate(s, wv, -45, block))
    with pytest.raises(ValueError):
        sess.volume(blocks[0][0][..., :-1])
    with pytest.raises(ValueError):
        sess.gate_(blocks[0][0])


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_python_refuses_bad_arguments():
    from ddsp_svc_amd import core, features
    x = torch.zeros(2, 1000)
    for bad in (lambda: features.volume(x, 160.5), lambda: features.volume(x, 0), lambda: features.volume(x[:, :80], 160),
                lambda: features.volume(x.double(), 160), lambda: features.volume(x[None], 160),
                lambda: features.gate(x, torch.zeros(2, 10), -45, 99), lambda: features.gate(x, torch.zeros(2, 10), -45, 100, dilate=65),
                lambda: features.gate(x, torch.zeros(2, 10), -45, 100, dilate=-1), lambda: features.gate(x, torch.zeros(2, 10), -45, 0),
                lambda: features.gate(x, torch.zeros(2, 10), -45, 100, out=torch.zeros(2, 999)),
                lambda: features.gate(x[0], torch.zeros(2, 10), -45, 100), lambda: features.silence_mask(torch.zeros(2, 3, 4), -45),
                lambda: features.decode_salience(torch.zeros(1, 5, 359)), lambda: features.decode_salience(torch.zeros(5, 360)),
                lambda: features.decode_salience(torch.zeros(1, 5, 360), center=torch.zeros(1, 4, dtype=torch.int64)),
                lambda: features.decode_salience(torch.zeros(1, 5, 360), center=torch.zeros(1, 5)),
                lambda: features.f0_track(x, 0.01, 512, SR, 10, mode="cubic"), lambda: features.f0_track(x, 0.0, 512, SR, 10),
                lambda: features.f0_track(x, 0.01, 512, SR, 0), lambda: features.f0_track(x, 0.01, 512, SR, 10, start_frame=11),
                lambda: features.f0_track(x, 0.01, 512, SR, 10, start_frame=-1), lambda: features.f0_track(x[:, :0], 0.01, 512, SR, 10),
                lambda: features.f0_track(x.long(), 0.01, 512, SR, 10),
                lambda: features.StreamingFeatures(1, 100, 512, 10, 0.01, SR, 512, -45), lambda: features.StreamingFeatures(0, 9000, 512, 10, 0.01, SR, 512, -45),
                lambda: features.StreamingFeatures(1, 9000, 512.5, 10, 0.01, SR, 512, -45),
                lambda: core.MedianPool1d(x, 17), lambda: core.MaskedAvgPool1d(x, 0), lambda: core.MedianPool1d(x[:, :4], 9),
                lambda: core.MaskedAvgPool1d(x[0], 3), lambda: core.MedianPool1d(x.double(), 3)):
        with pytest.raises(ValueError):
            bad()


def test_features_abi_argument_errors():
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    p, q, ws = 4096, 8192, 65536                        # never dereferenced: every call below fails its checks first

    def vol(audio=p, ld=1000, B=1, T=1000, hop=160, out=q):
        return lib.ddsp_hip_volume(audio, ld, B, T, hop, out, None)
    assert vol(T=0) == EINVAL and vol(hop=0) == EINVAL and vol(B=-1) == EINVAL and vol(audio=None) == EINVAL and vol(out=None) == EINVAL
    assert vol(T=80, hop=160) == ESHAPE and vol(T=81, hop=161) == ESHAPE and vol(B=2, ld=999) == EINVAL and vol(B=70000) == ESHAPE
    assert vol(B=0) == 0

    def gate(sig=p, ld=1000, vol=p, B=1, F=10, block=100, thr=0.01, d=4, out=q, ldo=1000):
        return lib.ddsp_hip_gate(sig, ld, vol, B, F, block, thr, d, out, ldo, None)
    assert gate(F=0) == EINVAL and gate(block=0) == EINVAL and gate(d=-1) == EINVAL and gate(thr=float("nan")) == EINVAL
    assert gate(d=65) == ESHAPE and gate(B=2, ld=999) == EINVAL and gate(B=2, ldo=999) == EINVAL
    assert gate(sig=None) == EINVAL and gate(vol=None) == EINVAL and gate(out=None) == EINVAL and gate(B=0) == 0

    assert lib.ddsp_hip_decode_salience(p, -1, None, 0.03, q, None) == EINVAL
    assert lib.ddsp_hip_decode_salience(None, 4, None, 0.03, q, None) == EINVAL
    assert lib.ddsp_hip_decode_salience(p, 4, None, 0.03, None, None) == EINVAL
    assert lib.ddsp_hip_decode_salience(p, 0, None, 0.03, q, None) == 0

    need = lib.ddsp_hip_f0_track_workspace_bytes(2, 100, 61)
    assert need == 2 * (400 + 400 + 496)
    assert lib.ddsp_hip_f0_track_workspace_bytes(0, 100, 61) == 0 and lib.ddsp_hip_f0_track_workspace_bytes(1, 0, 61) == 0
    assert lib.ddsp_hip_f0_track_workspace_bytes(1, 100, 0) == 0 and lib.ddsp_hip_f0_track_workspace_bytes(1, (1 << 30) + 1, 5) == 0

    def track(src=p, ld=100, B=2, N=100, period=0.01, hop=512.0, sr=44100.0, n=61, start=0, mode=0, uv=0, out=q, w=ws, wb=1 << 20):
        return lib.ddsp_hip_f0_track(src, ld, B, N, period, hop, sr, n, start, mode, uv, 65.0, out, w, wb, None)
    assert track(N=0) == EINVAL and track(n=0) == EINVAL and track(start=-1) == EINVAL and track(start=62) == EINVAL
    assert track(period=0.0) == EINVAL and track(hop=0.0) == EINVAL and track(sr=-1.0) == EINVAL and track(mode=2) == EINVAL
    assert track(ld=99) == EINVAL and track(src=None) == EINVAL and track(out=None) == EINVAL
    assert track(N=(1 << 30) + 1, ld=1 << 31) == ESHAPE
    assert track(w=None) == EWS and track(wb=need - 1) == EWS and track(w=ws + 8) == EINVAL and track(B=0) == 0

    def pool(x=p, B=1, N=100, k=4, y=q):
        return lib.ddsp_hip_pool1d(x, B, N, k, 0, y, None)
    assert pool(N=0) == EINVAL and pool(x=None) == EINVAL and pool(y=p) == EINVAL and pool(B=-1) == EINVAL
    assert pool(k=0) == ESHAPE and pool(k=17) == ESHAPE and pool(N=4, k=9) == ESHAPE and pool(B=0) == 0


# ---- the patch ----------------------------------------------------------------------------------------------------------------
def test_patch_rebinds_the_reference_names_and_unpatch_restores_them(monkeypatch):
    from ddsp_svc_amd import features
    calls = []

    def masked(x, kernel_size):
        calls.append("avg")
        return x

    def median(x, kernel_size):
        calls.append("median")
        return x

    def decode(hidden, center=None, thred=0.03):
        calls.append("decode")
        return hidden[..., 0].squeeze(0).cpu().numpy()
    mods = {"ddsp": types.ModuleType("ddsp"), "ddsp.core": types.ModuleType("ddsp.core"),
            "ddsp.vocoder": types.ModuleType("ddsp.vocoder"), "encoder": types.ModuleType("encoder"),
            "encoder.rmvpe": types.ModuleType("encoder.rmvpe"), "encoder.rmvpe.utils": types.ModuleType("encoder.rmvpe.utils"),
            "encoder.rmvpe.inference": types.ModuleType("encoder.rmvpe.inference")}
    for name, m in mods.items():
        if "." not in name or name == "encoder.rmvpe":
            m.__path__ = []
        monkeypatch.setitem(sys.modules, name, m)
    rcore, rvoc, rutils, rinf = (mods[k] for k in ("ddsp.core", "ddsp.vocoder", "encoder.rmvpe.utils", "encoder.rmvpe.inference"))
    rcore.MaskedAvgPool1d, rcore.MedianPool1d = masked, median
    rvoc.MaskedAvgPool1d, rvoc.MedianPool1d = masked, median          # ddsp/vocoder.py:16 imports both by name
    rutils.to_local_average_f0 = rinf.to_local_average_f0 = decode
    monkeypatch.setattr(features, "_REBOUND", [])
    monkeypatch.setattr(features, "_PARKED", [])
    rebound = features.patch_reference_features()
    assert sorted(rebound) == sorted([("ddsp.core", "MaskedAvgPool1d"), ("ddsp.core", "MedianPool1d"),
                                      ("ddsp.vocoder", "MaskedAvgPool1d"), ("ddsp.vocoder", "MedianPool1d"),
                                      ("encoder.rmvpe.utils", "to_local_average_f0"),
                                      ("encoder.rmvpe.inference", "to_local_average_f0")])
    assert rvoc.MaskedAvgPool1d is rcore.MaskedAvgPool1d is not masked and rinf.to_local_average_f0 is rutils.to_local_average_f0
    assert rcore._reference_MedianPool1d is median and rutils._reference_to_local_average_f0 is decode
    assert features.patch_reference_features() == []                # idempotent
    x = torch.zeros(1, 8)                                           # CPU tensors keep the reference's own code
    assert rvoc.MaskedAvgPool1d(x, 4) is x and rvoc.MedianPool1d(x, 4) is x
    out = rinf.to_local_average_f0(torch.zeros(1, 5, 360), thred=0.03)
    assert calls == ["avg", "median", "decode"] and isinstance(out, np.ndarray) and out.shape == (5,)
    features.unpatch_reference_features()
    assert rcore.MaskedAvgPool1d is masked and rvoc.MedianPool1d is median and rinf.to_local_average_f0 is decode
    assert rutils.to_local_average_f0 is decode and not hasattr(rcore, "_reference_MedianPool1d")


@pytest.mark.gpu
def test_patched_reference_names_run_on_hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddsp_svc_amd import core, features
    calls = []
    orig = lambda *a, **k: calls.append(1)
    pool = features._dispatch_pool(orig, core.MedianPool1d)
    x = torch.rand(2, 40, device="cuda")
    assert torch.equal(pool(x, 4), core.MedianPool1d(x, 4)) and calls == []
    pool(x, 17)
    assert calls == [1]
    h = _t(_salience(1, 7, 11), torch.device("cuda:0"))
    got = features._dispatch_decode(orig)(h, thred=0.03)
    assert isinstance(got, np.ndarray) and got.shape == (7,) and calls == [1]
    assert np.array_equal(got, features.decode_salience(h)[0].cpu().numpy())
