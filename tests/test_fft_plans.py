"""The in-register / LDS FFT plans of ddsp_svc_amd/csrc/fft_r.h (the building blocks of k_fir_blk, k_stft_filter, k_mel) on
their own (tests/device_units/units.hip), under the CPU emulator -- the plain C++ twins -- and on the MI355X -- the packed-f32 /
DPP assembly that ships --, against numpy.fft in float64: the full three-exchange transform at 512, 1024, 2048 and 4096 points, the
two-exchange pair that stays in the scrambled layout S (forward_s with and without the pruned first pass, transposed), and
the two lockstep forms, which must equal their separate transforms bit for bit (same arithmetic, shared barriers).  The bit-for-bit
equalities are taken on one device; nothing here compares GPU bits with emulator bits (the twiddles come from the sincospif of two
different math libraries)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.device_units.backend import BACKENDS, cases, load

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def plans(request):
    """run(R, mode, a, b) -> (out, out2) on the backend the test is parametrized with: a and b are one input of 512 R complex
    words or a batch of them (one workgroup each, one launch)"""
    u = load(request.param)

    def run(R, mode, a, b=None):
        n = 512 * R
        a = np.ascontiguousarray(a, dtype=np.complex64)
        batch = a.size // n
        ta = u.to(a)
        tb = u.to(np.ascontiguousarray(b, dtype=np.complex64)) if b is not None else ta
        o1 = u.zeros(a.shape, torch.complex64)
        o2 = u.zeros(a.shape, torch.complex64) if b is not None else o1      # the one-input modes never touch in2 / out2
        u.call("du_fft_plan", R, mode, batch, ta, tb, o1, o2)
        return u.numpy(o1), u.numpy(o2)
    run.backend = u
    return run


def _rand(n, seed, half=False):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    if half:
        z[n // 2:] = 0
    return z


def _close(got, ref):
    ref = ref.astype(np.complex128)
    return np.sqrt(np.mean(np.abs(got - ref) ** 2)) <= 3e-7 * np.sqrt(np.mean(np.abs(ref) ** 2))


@pytest.mark.parametrize("plans,R", cases([1, 2, 4, 8]), indirect=["plans"])
def test_full_transform(plans, R):
    z = _rand(512 * R, R)
    assert _close(plans(R, 0, z)[0], np.fft.fft(z.astype(np.complex128)))


@pytest.mark.parametrize("plans,R", cases([1, 2, 4, 8]), indirect=["plans"])
def test_lockstep_pair_and_zero_padded_first_pass(plans, R):
    """forward2 = two forward calls behind shared barriers, bit for bit; the pruned first pass (upper half of the input zero,
    never read) against numpy and, in lockstep, against itself."""
    n = 512 * R
    a, b = _rand(n, 30 + R), _rand(n, 40 + R)
    one_a, one_b = plans(R, 0, a)[0], plans(R, 0, b)[0]
    two_a, two_b = plans(R, 10, a, b)
    assert np.array_equal(one_a, two_a) and np.array_equal(one_b, two_b)
    ah, bh = _rand(n, 50 + R, half=True), _rand(n, 60 + R, half=True)
    pruned = plans(R, 12, ah)[0]
    assert _close(pruned, np.fft.fft(ah.astype(np.complex128)))
    pa, pb = plans(R, 11, ah, bh)
    assert np.array_equal(pa, pruned) and np.array_equal(pb, plans(R, 12, bh)[0])


@pytest.mark.parametrize("plans", BACKENDS, indirect=True)
def test_layout_s_pair(plans):
    z = _rand(1024, 10)
    zh = _rand(1024, 11, half=True)
    assert _close(plans(2, 1, z)[0], np.fft.fft(z.astype(np.complex128)))
    assert _close(plans(2, 2, zh)[0], np.fft.fft(zh.astype(np.complex128)))
    assert _close(plans(2, 3, z)[0], np.fft.fft(z.astype(np.complex128)))          # the transposed factorisation is the DFT itself
    # forward_s then transposed of the conjugate = N times the input, conjugated (the inverse-by-forward trick of the kernels)
    spec = plans(2, 1, z)[0]
    back = np.conj(plans(2, 3, np.conj(spec))[0]) / 1024
    assert _close(back, z)


@pytest.mark.parametrize("plans", BACKENDS, indirect=True)
def test_lockstep_forms_equal_their_parts(plans):
    a, b = _rand(1024, 20, half=True), _rand(1024, 21, half=True)
    one_a, one_b = plans(2, 2, a)[0], plans(2, 2, b)[0]
    two_a, two_b = plans(2, 4, a, b)
    assert np.array_equal(one_a, two_a) and np.array_equal(one_b, two_b)
    v = _rand(1024, 22)
    inv, fwd = plans(2, 5, v, b)
    assert np.array_equal(inv, plans(2, 3, v)[0]) and np.array_equal(fwd, one_b)
    # the three-buffer form (the tap transform one exchange behind the inverse): the same arithmetic again
    inv3, fwd3 = plans(2, 13, v, b)
    assert np.array_equal(inv3, inv) and np.array_equal(fwd3, one_b)


@pytest.mark.parametrize("plans", BACKENDS, indirect=True)
def test_sign_carrying_layout(plans):
    """layout S- (one v_fmac_f32 with a DPP operand per value in the lane-pair step; odd threads hold negated values): with the
    sign undone the transforms are those of the plain layout -- the lane-pair step computes a0 - a1 as -(a1 - a0), exactly"""
    a, b = _rand(1024, 30, half=True), _rand(1024, 31, half=True)
    v = _rand(1024, 32)
    assert np.array_equal(plans(2, 6, a)[0], plans(2, 2, a)[0])
    assert np.array_equal(plans(2, 7, v)[0], plans(2, 3, v)[0])
    two_a, two_b = plans(2, 8, a, b)
    assert np.array_equal(two_a, plans(2, 2, a)[0]) and np.array_equal(two_b, plans(2, 2, b)[0])
    inv, fwd = plans(2, 9, v, b)
    assert np.array_equal(inv, plans(2, 3, v)[0]) and np.array_equal(fwd, plans(2, 2, b)[0])
    inv, fwd = plans(2, 14, v, b)
    assert np.array_equal(inv, plans(2, 3, v)[0]) and np.array_equal(fwd, plans(2, 2, b)[0])


@pytest.mark.parametrize("plans", BACKENDS, indirect=True)
def test_padded_row_plan(plans):
    """fft_1024p.h (k_fir_blk6): the same transforms on padded exchange rows -- one base register per exchange instead of XOR
    swizzles -- bit for bit; and its one-base form of the mirrored read against parked(-k) for every thread and slot"""
    a, b = _rand(1024, 70, half=True), _rand(1024, 71, half=True)
    v = _rand(1024, 72)
    assert np.array_equal(plans(2, 15, a)[0], plans(2, 2, a)[0])
    inv, fwd = plans(2, 16, v, b)
    assert np.array_equal(inv, plans(2, 3, v)[0]) and np.array_equal(fwd, plans(2, 2, b)[0])
    assert float(np.abs(plans(2, 17, a)[0][:128]).sum()) == 0.0


@pytest.mark.parametrize("plans,R", cases([1, 2, 4, 8]), indirect=["plans"])
def test_unit_impulses_give_the_twiddles(plans, R):
    """What random inputs average away: a unit impulse at index j transforms to W_N^(jk), so every bin shows one product of the
    plan's twiddles on its own.  Bar: a bin is the product of at most four unit-modulus factors, each within 2^-23 of its exact
    value, through at most four complex products that each add at most sqrt(2) 2^-23: 4 (1 + sqrt(2)) 2^-23 = 1.15e-6, asserted as
    1.2e-6 absolute per bin (a wrong twiddle index at N = 4096 is off by at least 1.5e-3).  Every j on the GPU, one launch per R;
    j = 0, 1, N/2, N-1 and 64 seeded others under the emulator."""
    n = 512 * R
    if plans.backend.name == "gpu":
        js = np.arange(n)
    else:
        js = np.concatenate([[0, 1, n // 2, n - 1], np.random.default_rng(90 + R).integers(0, n, 64)])
    z = np.zeros((len(js), n), np.complex64)
    z[np.arange(len(js)), js] = 1
    got = plans(R, 0, z)[0]
    w = np.exp(-2j * np.pi * np.arange(n) / n)
    k = np.arange(n)
    worst = 0.0
    for lo in range(0, len(js), 256):
        ref = w[(js[lo:lo + 256, None] * k[None, :]) % n]
        worst = max(worst, float(np.abs(got[lo:lo + 256] - ref).max()))
    print("N = %d: worst bin error over %d impulses %.3e" % (n, len(js), worst))
    assert worst <= 1.2e-6


def test_emulator_selftest():
    """the emulator's own kernels (LDS reversal across a barrier, a wave scan through shuffles, one f32 MFMA, work-items
    that leave before a barrier): tests/hipemu/selftest.hip"""
    from tests.hipemu import build as emu
    emu.build()
    out = os.path.join(emu.OUT, "libemu_selftest.so")
    src = os.path.join(HERE, "hipemu", "selftest.hip")
    obj = os.path.join(emu.OUT, "selftest.o")
    if not os.path.exists(out) or os.path.getmtime(src) > os.path.getmtime(out):
        subprocess.run([emu._clang(), "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-I", emu.HERE, "-I", emu.CSRC,
                        "-Wno-unknown-attributes", "-Wno-unused-function", "-c", src, "-o", obj], check=True)
        subprocess.run([emu._clang(), "-shared", "-fPIC", obj, os.path.join(emu.OUT, "hipemu.o"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_selftest.restype = ctypes.c_int
    assert L.emu_selftest() == 0
