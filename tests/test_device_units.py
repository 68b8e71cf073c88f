"""The building blocks one layer below the kernels -- the packed complex helpers of fft2048.h and the wave scans, buffer
descriptors and hardware-math wrappers of ddsp_common.h -- called one at a time by the kernels of tests/device_units/units.hip.
That source is built twice: the ``emu`` leg runs the plain C++ twins under the CPU emulator (whose DPP, buffer and transcendental
intrinsics are the project's own reading of the ISA manual), the ``gpu`` leg runs the ``__HIP_DEVICE_COMPILE__`` bodies that ship,
on the MI355X.  Both legs face the same float64 references and the same exact expectations, and the helpers' twin outputs are pinned
in tests/golden/device_units.npz so that the GPU is held to the twin's bits.  The FFT plans built from these pieces:
tests/test_fft_plans.py."""
import os

import numpy as np
import pytest
import torch

from tests.device_units import helper_cases as hc
from tests.device_units.backend import BACKENDS, units  # noqa: F401

both = pytest.mark.parametrize("units", BACKENDS, indirect=True)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "device_units.npz")))


# ---------------------------------------------------------------- packed complex helpers
def _mismatch(got, want):
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = np.argwhere((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w)))
    return "%d of %d components differ, first at (record, slot, half) %s: got %r, want %r" % (
        len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]) if len(bad) else ""


@both
@pytest.mark.parametrize("name", list(hc.HELPERS))
def test_helper_gives_the_twins_bits(units, name, golden):
    """Both bodies are the same IEEE operations in the same order (v_pk_mul then v_pk_fma against * then an elementwise fma), so the
    twin's outputs -- the fixture, which the emulator leg reproduces -- are what the GPU must give, bit for bit, on 4096 seeded
    normal operands and on every combination of +-0, +-1, +-inf (hc.random_records / hc.special_records)."""
    rec = hc.random_records(name)
    assert not _mismatch(hc.run(units, name, rec), hc.unpack(name, rec, golden["rand_" + name]))
    assert not _mismatch(hc.run(units, name, hc.special_records(name)), golden["spec_" + name])


@both
@pytest.mark.parametrize("name", list(hc.HELPERS))
def test_helper_against_float64(units, name):
    """Independently of the twin: every output component within 2^-23 of the sum of the absolute values of its exact terms (one
    rounding per multiply and per add or fma) of its float64 value; the pure add / swizzle helpers and swap_scale, one rounding
    each, equal to the correctly rounded float32 result -- on the special values too."""
    rec = hc.random_records(name)
    got = hc.run(units, name, rec)
    val, mag = hc.model(name, rec)
    err = np.abs(got.astype(np.float64) - val)
    print("%s: worst error %.3f of 2^-23 sum|terms|" % (name, float((err / (2.0 ** -23 * mag + 1e-300)).max())))
    assert np.all(err <= 2.0 ** -23 * mag)
    if name in hc.EXACT:
        assert not _mismatch(got, hc.correctly_rounded(name, rec))
        spec = hc.special_records(name)
        assert not _mismatch(hc.run(units, name, spec), hc.correctly_rounded(name, spec))


# ---------------------------------------------------------------- wave scans and reductions
def _wave_inputs(kind):
    """rows of 64 lanes: 8 random rows, then one row per lane with that lane alone non-zero (which lanes each DPP step reaches)"""
    rng = np.random.default_rng(7)
    single = np.zeros((64, 64))
    single[np.arange(64), np.arange(64)] = np.arange(64) + 1.0
    if kind == "f64":
        return np.concatenate([rng.integers(0, 1 << 24, (8, 64)) * 2.0 ** -24,        # multiples of 2^-24 below 1 (sinegen's argument)
                               rng.integers(0, (1 << 40) + 1, (8, 64)).astype(np.float64), single])
    if kind == "f32":
        return np.concatenate([rng.integers(0, 1 << 18, (16, 64)).astype(np.float64), single]).astype(np.float32)
    top = np.arange(64)
    high = rng.integers(0, (1 << 32) - 1, (64, 64))          # anything, the maximum 2^32 - 1 in lane `row`
    high[top, top] = (1 << 32) - 1
    low = rng.integers(0, 1 << 31, (64, 64))                 # below 2^31, the maximum exactly 2^31: negative to a signed compare
    low[top, top] = 1 << 31
    return np.concatenate([rng.integers(0, 1 << 32, (16, 64)), high, low]).astype(np.uint32)


@both
@pytest.mark.parametrize("waves_per_block", [1, 4])
def test_wave_scans_f64(units, waves_per_block):
    """wave_incl_scan / wave_excl_scan / wave_sum: every partial sum of these inputs is exact in float64, so the bar is equality
    with numpy.cumsum -- which makes GPU and emulator agree bit for bit; four waves per workgroup must not leak into each other"""
    v = _wave_inputs("f64")
    incl, excl, tot = (units.zeros(v.shape, torch.float64) for _ in range(3))
    units.call("du_wave_f64", units.to(v), incl, excl, tot, len(v), waves_per_block)
    want = np.cumsum(v, axis=1)
    for got, ref, what in ((incl, want, "wave_incl_scan"), (excl, want - v, "wave_excl_scan"), (tot, np.repeat(want[:, -1:], 64, 1), "wave_sum")):
        got = units.numpy(got)
        bad = np.argwhere(got != ref)
        assert not len(bad), "%s: row %d lane %d: got %r, want %r" % (what, *bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


@both
@pytest.mark.parametrize("waves_per_block", [1, 4])
def test_wave_sum_dpp_f32(units, waves_per_block):
    """integer-valued inputs below 2^18: 64 of them sum exactly in float32 in any order"""
    v = _wave_inputs("f32")
    got = units.zeros(v.shape, torch.float32)
    units.call("du_wave_f32", units.to(v), got, len(v), waves_per_block)
    assert np.array_equal(units.numpy(got), np.repeat(v.astype(np.float64).sum(1, keepdims=True), 64, 1).astype(np.float32))


@both
@pytest.mark.parametrize("waves_per_block", [1, 4])
def test_wave_max_dpp_unsigned(units, waves_per_block):
    """values at and above 2^31 (the function goes through (int) casts), the maximum in each of the 64 lanes in turn"""
    v = _wave_inputs("u32")
    got = units.zeros(v.shape, torch.int32)
    units.call("du_wave_u32", units.to(v.view(np.int32)), got, len(v), waves_per_block)
    assert np.array_equal(units.numpy(got).view(np.uint32), np.repeat(v.max(1, keepdims=True), 64, 1))


# ---------------------------------------------------------------- hardware-math wrappers
FN = {"tanh_hw": 0, "exp_hw": 1, "sin_turns": 2, "sin_turns2.x": 3, "sin_turns2.y": 4, "sinc_f32": 5, "div_pos": 6, "cis_pi.x": 7,
      "cis_pi.y": 8}


def _math(units, fn, a, b=None):
    a = np.ascontiguousarray(a, np.float32)
    ta = units.to(a)
    tb = units.to(np.ascontiguousarray(b, np.float32)) if b is not None else ta
    out = units.zeros(a.shape, torch.float32)
    units.call("du_math", FN[fn], ta, tb, out, a.size)
    return units.numpy(out)


def _points(units):
    """2^20 points per function on the GPU, which measures the hardware; 2^14 under the emulator, which checks the algebra on libm"""
    return 1 << 20 if units.name == "gpu" else 1 << 14


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@both
def test_tanh_hw(units):
    """|x| <= 50, half of the points dense near 0: absolute error <= 1.5e-7 (the bound of the header comment); signed zeros and
    infinities; +-1 exactly beyond 44.  The relative error near |x| = 1e-4 is printed, not asserted: the 1 - 2 / (e + 1) form
    loses the small results' relative accuracy by design."""
    n, rng = _points(units), np.random.default_rng(11)
    x = np.concatenate([rng.uniform(-50, 50, n // 2), rng.choice([-1.0, 1.0], n // 2) * 10.0 ** rng.uniform(-8, 0, n // 2)]).astype(np.float32)
    got, ref = _math(units, "tanh_hw", x), np.tanh(x.astype(np.float64))
    print("tanh_hw: worst abs error %.3e over %d points" % (np.abs(got - ref).max(), n))
    assert np.abs(got - ref).max() <= 1.5e-7
    far = np.abs(x) > 44
    assert far.any() and np.array_equal(got[far], np.sign(x[far]))
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 44.5, -44.5, 1e30, -1e30], np.float32)
    assert np.array_equal(_bits(_math(units, "tanh_hw", edge)), _bits(np.array([0.0, -0.0, 1, -1, 1, -1, 1, -1], np.float32)))
    small = (rng.choice([-1.0, 1.0], 4096) * rng.uniform(0.9e-4, 1.1e-4, 4096)).astype(np.float32)
    rel = np.abs(_math(units, "tanh_hw", small) / np.tanh(small.astype(np.float64)) - 1)
    print("tanh_hw: worst relative error at |x| ~ 1e-4: %.3e" % rel.max())


@both
def test_exp_hw(units):
    """|x| <= 80: relative error <= 1.5 * 2^-23; the limits of torch.exp beyond the finite range.  The bar is derived, not measured:
    v_exp_f32 is specified to 1 ulp, i.e. 2^-23 relative, the final fma adds one rounding of 2^-24, and what the split of x log2(e)
    leaves (the residual's rounding, the dropped (r ln 2)^2 / 2) is below 1e-11.  A bar of 2^-23 alone, which is what "~1e-7" in the
    header comment amounted to, leaves the second rounding no room: the MI355X measures 1.354e-7 = 1.136 * 2^-23 over these 2^20
    points (libm's exp2f under the emulator: 1.107e-7), so the comment in ddsp_common.h now states the derived bound."""
    n, rng = _points(units), np.random.default_rng(12)
    x = rng.uniform(-80, 80, n).astype(np.float32)
    got, ref = _math(units, "exp_hw", x), np.exp(x.astype(np.float64))
    rel = np.abs(got / ref - 1)
    print("exp_hw: worst relative error %.3e = %.3f * 2^-23 over %d points" % (rel.max(), rel.max() * 2.0 ** 23, n))
    assert rel.max() <= 1.5 * 2.0 ** -23
    edge = np.array([88.74, 89, 100, 1e30, np.inf, -104.01, -150, -1e30, -np.inf, np.nan], np.float32)
    out = _math(units, "exp_hw", edge)
    assert np.all(out[:5] == np.inf) and np.array_equal(_bits(out[5:9]), np.zeros(4, np.uint32)) and np.isnan(out[9])
    tiny = np.linspace(-103, -88, 64).astype(np.float32)     # results below the normal range: kept or flushed, recorded as it is
    out = _math(units, "exp_hw", tiny)
    print("exp_hw: %d of %d denormal results come out as 0" % (int((out == 0).sum()), len(out)))
    assert np.all((out >= 0) & (out < 2.0 ** -126))


@both
def test_sin_turns(units):
    """|a| <= 805 (the sinusoid bank reaches 256 pi): absolute error <= 3.9e-7; sin_turns2 is sin_turns per half, bit for bit"""
    n, rng = _points(units), np.random.default_rng(13)
    a, b = rng.uniform(-805, 805, n).astype(np.float32), rng.uniform(-805, 805, n).astype(np.float32)
    one_a, one_b = _math(units, "sin_turns", a), _math(units, "sin_turns", b)
    for x, got in ((a, one_a), (b, one_b)):
        err = np.abs(got - np.sin(x.astype(np.float64))).max()
        print("sin_turns: worst abs error %.3e over %d points" % (err, n))
        assert err <= 3.9e-7
    assert np.array_equal(_bits(_math(units, "sin_turns2.x", a, b)), _bits(one_a))
    assert np.array_equal(_bits(_math(units, "sin_turns2.y", a, b)), _bits(one_b))


@both
def test_cis_pi(units):
    """the spectral filters' phase factor: (cos, sin) of the float32 product fl32(pi32 * p), the angle the reference's complex64
    exponential sees, for |pi p| <= 805, i.e. |p| <= 256 -- sin_turns' reduction and range, so sin_turns' bound: 3.9e-7 absolute"""
    n, rng = _points(units), np.random.default_rng(17)
    p = rng.uniform(-256, 256, n).astype(np.float32)
    ang = (np.float32(np.pi) * p).astype(np.float32).astype(np.float64)
    for fn, ref in (("cis_pi.x", np.cos(ang)), ("cis_pi.y", np.sin(ang))):
        err = np.abs(_math(units, fn, p) - ref).max()
        print("%s: worst abs error %.3e over %d points" % (fn, err, n))
        assert err <= 3.9e-7


@both
def test_sinc_f32(units):
    """|z| <= 300, a third of the points dense around |pi z| = 2 where the series hands over to the hardware sine: absolute error
    <= 2.4e-7 against sin(pi z) / (pi z) in float64; 1 at +-0"""
    n, rng = _points(units), np.random.default_rng(14)
    third = n // 3
    z = np.concatenate([rng.uniform(-300, 300, n - 2 * third), rng.uniform(-1, 1, third),
                        rng.choice([-1.0, 1.0], third) * (2 / np.pi) * (1 + rng.uniform(-1e-3, 1e-3, third))]).astype(np.float32)
    got, ref = _math(units, "sinc_f32", z), np.sinc(z.astype(np.float64))
    print("sinc_f32: worst abs error %.3e over %d points" % (np.abs(got - ref).max(), n))
    assert np.abs(got - ref).max() <= 2.4e-7
    assert np.array_equal(_math(units, "sinc_f32", np.array([0.0, -0.0], np.float32)), np.ones(2, np.float32))


@both
def test_div_pos(units):
    """the exciters' range, a in [0, 1] sr over b = f0 + 1e-3 with f0 in 12.5 .. 4400, 2^22 pairs: every quotient within 1 ulp of
    IEEE float32 division, and at most 1e-4 of them not the correctly rounded one (the header's rate is 1e-7; without the residual
    correction it is tens of per cent, so the cap catches a broken correction and leaves room for the documented rate)"""
    n, rng = 1 << 22, np.random.default_rng(15)
    a = (rng.uniform(0, 1, n) * 44100.0).astype(np.float32)
    b = (rng.uniform(12.5, 4400, n).astype(np.float32) + np.float32(1e-3)).astype(np.float32)
    got, ref = _math(units, "div_pos", a, b), a / b
    ulps = np.abs(_bits(got).astype(np.int64) - _bits(ref).astype(np.int64))
    share = float((ulps != 0).mean())
    print("div_pos: worst distance %d ulp, %d of %d (%.2e) not correctly rounded" % (ulps.max(), int((ulps != 0).sum()), n, share))
    assert ulps.max() <= 1 and share <= 1e-4


@both
def test_phase_term_is_ieee_division(units):
    """PhaseCfg::term on the inference path: f0.double() / sr through the reciprocal and one residual correction equals IEEE float64
    division bit for bit -- the header's exhaustive claim, pinned: 1.5 M seeded float32 f0 in [0, 5000] (64 K under the emulator)
    at each common sampling rate"""
    n = 1_500_000 if units.name == "gpu" else 1 << 16
    f0 = np.random.default_rng(16).uniform(0, 5000, n).astype(np.float32)
    f0[:2] = 0.0, 5000.0
    t, out = units.to(f0), units.zeros(n, torch.float64)
    for sr in (16000, 22050, 24000, 32000, 44100, 48000):
        units.call("du_phase_term", t, out, n, float(sr))
        want = f0.astype(np.float64) / float(sr)
        bad = np.flatnonzero(units.numpy(out).view(np.int64) != want.view(np.int64))
        assert not len(bad), "sr %d: %d of %d terms are not the IEEE quotient, first f0 = %r" % (sr, len(bad), n, f0[bad[0]])


# ---------------------------------------------------------------- BufF32
GUARD, SPAN = 128, 100                                       # guard floats on both sides of the descriptor's SPAN floats
OFFSETS = np.array([0, 1, SPAN // 2, SPAN - 1] + list(range(SPAN, SPAN + 65)), np.int32)      # the last float, then 0 .. 64 floats past the end


def _buf(units, op, tensor, n_floats):
    vals = np.arange(len(OFFSETS), dtype=np.float32) + 1000
    got = units.zeros(len(OFFSETS), torch.float32) - 1
    units.call("du_buf", op, tensor[GUARD:], n_floats, units.to(OFFSETS), units.to(vals), got, len(OFFSETS))
    return units.numpy(got), vals


@both
@pytest.mark.parametrize("n_floats", [SPAN, 0])
def test_buffer_descriptor_inside_one_allocation(units, n_floats):
    """A descriptor over the middle SPAN floats of a tensor with GUARD floats on both sides (every offset used stays inside that
    tensor: an access the hardware failed to drop would land in a guard and fail the assertion, nothing more).  ld / ld_nt: in-range
    floats come back, out-of-range ones read +0.0; st / st_nt: in-range floats are written, the guards stay; a descriptor of
    0 floats drops everything."""
    fill = np.arange(2 * GUARD + SPAN, dtype=np.float32) + 1
    inside = OFFSETS < n_floats
    for op in (0, 1):
        t = units.to(fill)
        got, _ = _buf(units, op, t, n_floats)
        assert np.array_equal(_bits(got), _bits(np.where(inside, fill[GUARD + OFFSETS], np.float32(0.0))))
        assert np.array_equal(units.numpy(t), fill)
    for op in (2, 3):
        t = units.to(fill)
        _, vals = _buf(units, op, t, n_floats)
        want = fill.copy()
        want[GUARD + OFFSETS[inside]] = vals[inside]
        assert np.array_equal(units.numpy(t), want)
