"""The phase state under ``infer``: sum first, scale once (csrc/ddsp_common.h, PhaseCfg; csrc/phase.hip, csrc/frame_phase.h).

Under ``infer`` the kernels of the shift form (hop a power of two up to 512) accumulate ``double(f0u)`` and multiply the SUM by
``RN(1 / sr)`` once; the general interpolation (hop 441, hop 1024 here) keeps the per-sample quotients.  Either way the frame totals,
``phase0`` and ``x`` are held to a host reference written here: the float32 upsampled values as the kernels form them, and the EXACT
sum of the correctly rounded quotients ``v / sr`` (integers, rounded once: what ``math.fsum`` returns).

Bounds.  No value of the state is more than 40 roundings deep (8 samples of a lane, 6 steps of a wave scan, one scaling, a scan chunk of
up to 5 totals, the 8 rounds of the scan over the 256 chunk sums, the chunk again), half an ulp each: 20 float64 ulp of the largest partial sum
that can stand in the chain -- for a frame total that total (all terms are >= 0), for ``phase0`` the utterance's last partial sum (an
exclusive prefix is formed as inclusive - own, so a small prefix carries the rounding of the larger inclusive sum).  ``x`` from
``want_x=True``: the project's 6e-8 cycles.

How many ``x`` values change their float32 bits against the per-sample-division form (the arithmetic before this change), from the
float64 host emulation of both forms below (lane sums, the DPP scan's association row_shr 1/2/4/8, row_bcast15, row_bcast31, the
Hillis-Steele frame scan, an exact fma), counted by ``test_bits_against_per_sample_division``:

    seed 77, F = 17 (the input of tests/test_front_same_bits.py)      0 of   8 704
    mixed / vibrato rows, B = 2, F = 17                               0 of  17 408
    mixed / vibrato rows, B = 2, F = 257                              2 of 263 168   (one float32 ulp, <= 2.4e-10 cycles)

``infer=False`` is the training path and must not move at all: ``phase0``, ``x`` and a CombSub signal against arrays recorded from the
parent commit's build on an MI355X (tests/golden/phase_parent_noinfer.npz, written by tests/golden/make_golden_phase_noinfer.py)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, dev  # noqa: F401

SR = 44100
ULPS = 20
X_TOL = 6e-8
NOINFER_FILE = "phase_parent_noinfer.npz"


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def f0_rows(kind, F, seed=5):
    """[2, F] float32: row 0 of the kind asked for, row 1 a vibrato"""
    t = np.arange(F, dtype=np.float64)
    vib = (220.0 * 2.0 ** (0.7 * np.sin(2 * np.pi * t / 23.0) / 12.0) + np.random.default_rng(seed).random(F)).astype(np.float32)
    if kind == "mixed":                                            # 0 (unvoiced), 1e-3 and 800 Hz meet inside single frames
        row = np.array([0.0, 1e-3, 800.0, 0.0, 800.0, 1e-3, 1e-3, 0.0], dtype=np.float32)[np.arange(F) % 8]
    elif kind == "const":
        row = np.full(F, 4400.0, dtype=np.float32)
    else:
        raise ValueError(kind)
    return np.stack([row, vib])


# ---- the host reference ---------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """float32 fma(a, b, c): the product and the sum in an 80-bit long double (48 + 24 bits fit 64), rounded once more"""
    return (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(np.float32)


def upsample_f32(row, hop):
    """[F] -> [F, hop] float32, the operations of csrc/ddsp_common.h (Upsampler): the shift form where hop is a power of two"""
    F = row.shape[0]
    row = row.astype(np.float32)
    scale = np.float32(F) / np.float32(F * hop)
    if hop > 1 and hop & (hop - 1) == 0 and F * hop <= 1 << 24:
        l1 = (np.arange(hop, dtype=np.float32) * scale)[None, :]
        b = row[:, None]
        c = row[np.minimum(np.arange(F) + 1, F - 1)][:, None]
        return _fma32(np.float32(1.0) - l1, np.broadcast_to(b, (F, hop)), l1 * c)
    t = np.arange(F * hop)
    src = scale * t.astype(np.float32)
    k = np.minimum(src.astype(np.int64), F)
    l1 = np.clip(src - k.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    l0 = np.float32(1.0) - l1
    k1 = k + (k < F)
    i0, i1 = np.minimum(k, F - 1), np.minimum(k1, F - 1)
    return _fma32(l0, row[i0], l1 * row[i1]).reshape(F, hop)


SCALE_BITS = 200                                                    # every term is a multiple of 2^-200 (v / sr >= 2^-149 / 2^16, 53 bits)


def _as_ints(terms):
    """float64 terms >= 0 -> Python integers, term * 2^SCALE_BITS (exact)"""
    m, e = np.frexp(terms)
    mi = np.round(m * 2.0 ** 53).astype(np.int64)
    sh = e.astype(np.int64) - 53 + SCALE_BITS
    assert (sh[mi != 0] >= 0).all()
    return [int(a) << int(s) if a else 0 for a, s in zip(mi.tolist(), sh.tolist())]


def _to_float(i):
    return i / (1 << SCALE_BITS)                                    # int / int: correctly rounded


@functools.lru_cache(maxsize=None)
def reference(kind, F, hop, seed=5):
    """per utterance: the upsampled float32 values, the frame totals and the exclusive frame prefixes (exact sums of RN(v / sr), rounded
    once), the largest partial sum, and the exact fraction of a cycle of the inclusive prefix at every sample"""
    f0 = f0_rows(kind, F, seed)
    return f0, [_reference_row(row, hop) for row in f0]


def _reference_row(row, hop):
    F = row.shape[0]
    v = upsample_f32(row, hop)
    terms = v.astype(np.float64) / float(SR)
    ints = np.array(_as_ints(terms.reshape(-1)), dtype=object).reshape(F, hop)
    totals_i = ints.sum(axis=1)
    prefix_i = np.concatenate([[0], np.cumsum(totals_i)])
    incl_i = np.cumsum(ints.reshape(-1))                            # the running sum at every sample (Python integers)
    one = 1 << SCALE_BITS
    frac = np.array([_to_float(int(i) % one) for i in incl_i])      # exact wrap, rounded once
    return dict(v=v, totals=np.array([_to_float(int(i)) for i in totals_i]),
                phase0=np.array([_to_float(int(i)) for i in prefix_i[:F]]), largest=_to_float(int(prefix_i[F])), frac=frac)


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
def run_phase(dev, f0, hop, ip=None, infer=True, want_x=False, sr=SR):
    """ddsp_hip_phase with the frame totals kept: (sums, phase0, phase_frames, x or None) as numpy arrays"""
    from ddsp_svc_amd import _ffi
    from ddsp_svc_amd._ffi import ptr
    B, F = f0.shape
    f0t = torch.from_numpy(np.ascontiguousarray(f0)).to(dev)
    ipt = None if ip is None else torch.from_numpy(np.asarray(ip, dtype=np.float32)).to(dev)
    sums = torch.full((B, F), float("nan"), dtype=torch.float64, device=dev)
    phase0 = torch.full((B, F), float("nan"), dtype=torch.float64, device=dev)
    pf = torch.empty(B, F, 1, dtype=torch.float32, device=dev)
    x = torch.empty(B, F * hop, dtype=torch.float32, device=dev) if want_x else None
    _ffi.check(_ffi.lib().ddsp_hip_phase(ptr(f0t), ptr(ipt), B, F, hop, float(sr), int(infer), ptr(sums), ptr(phase0), ptr(pf), ptr(x),
                                         _ffi.stream_of(f0t)))
    return sums.cpu().numpy(), phase0.cpu().numpy(), pf.cpu().numpy(), None if x is None else x.cpu().numpy()


IP = np.array([1.25, -2.5], dtype=np.float32)                       # radians

CASES = [("mixed", F, 512, F in (2, 257, 1025)) for F in (1, 2, 17, 257, 1024, 1025)] + [
    ("mixed", 17, 512, True),                                       # B = 2 with AND without initial_phase at one shape
    ("const", 17, 512, False),
    ("mixed", 17, 441, True),                                       # the general interpolation
    ("mixed", 17, 1024, False),                                     # SPL = 16
]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("small_path", [0, 1])                      # 0: one launch where the shape allows it; 1: the two-launch form
@pytest.mark.parametrize("kind,F,hop,with_ip", CASES)
def test_state_and_x_against_exact_sums(dev, knobs, kind, F, hop, with_ip, small_path):
    f0, ref = reference(kind, F, hop)
    ip = IP if with_ip else None
    knobs("SMALL_PATH", small_path)
    sums, phase0, _, _ = run_phase(dev, f0, hop, ip)
    _, phase0_x, _, x = run_phase(dev, f0, hop, ip, want_x=True)
    for b, r in enumerate(ref):
        e_tot = np.abs(sums[b] - r["totals"]) / ulp(r["totals"])
        e_p0 = np.abs(phase0[b] - r["phase0"]) / ulp(r["largest"])
        e_p0x = np.abs(phase0_x[b] - r["phase0"]) / ulp(r["largest"])
        cyc = r["frac"] + (float(IP[b]) / 2.0 / math.pi if with_ip else 0.0)
        d = x[b].astype(np.float64) - cyc
        e_x = np.abs(d - np.rint(d))                                # on the circle: x and the reference may wrap on either side of 0.5
        print("%s F=%d hop=%d ip=%d small_path=%d b=%d: totals %.2f ulp, phase0 %.2f / %.2f ulp of the largest partial sum, x %.3g cycles"
              % (kind, F, hop, with_ip, small_path, b, e_tot.max(), e_p0.max(), e_p0x.max(), e_x.max()))
        assert phase0[b, 0] == 0.0
        assert e_tot.max() <= ULPS and e_p0.max() <= ULPS and e_p0x.max() <= ULPS
        assert e_x.max() <= X_TOL
        assert np.abs(x[b]).max() <= 0.5


# ---- the scan alone -------------------------------------------------------------------------------------------------------------
SCAN_F = (1, 63, 64, 65, 255, 256, 257, 1024)                        # the wave and chunk edges of the 256 chunk sums


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("small_path", [0, 1])
@pytest.mark.parametrize("F", SCAN_F)
@pytest.mark.parametrize("pattern", ["ones", "alternating"])
def test_scan_is_exact_on_dyadic_totals(dev, knobs, F, pattern, small_path):
    """hop 2 at a sampling rate of 2: a frame's samples are f0[f] and (f0[f] + f0[f+1]) / 2, its total (3 f0[f] + f0[f+1]) / 4 -- with
    f0 = 1 every total is 1.0, with powers of two of alternating sign the totals are dyadic numbers of alternating sign and the prefixes
    cancel; every partial sum is exact in float64 whatever its association, so phase0 must be EXACT"""
    if pattern == "ones":
        f0 = np.ones((2, F), dtype=np.float32)
    else:
        e = (np.arange(F) * 7) % 11
        f0 = np.stack([(-1.0) ** np.arange(F) * 2.0 ** e, (-1.0) ** (np.arange(F) + 1) * 2.0 ** (10 - e)]).astype(np.float32)
    nxt = f0[:, np.minimum(np.arange(F) + 1, F - 1)]
    totals = (3.0 * f0.astype(np.float64) + nxt) / 4.0
    want = np.concatenate([np.zeros((2, 1)), np.cumsum(totals, axis=1)[:, :-1]], axis=1)      # exact: integers / 4 below 2^20
    knobs("SMALL_PATH", small_path)
    sums, phase0, _, _ = run_phase(dev, f0, 2, sr=2)
    assert np.array_equal(sums, totals)
    assert np.array_equal(phase0, want)
    if pattern == "ones":
        assert np.array_equal(phase0[0], np.arange(F, dtype=np.float64))


# ---- float32 bits of x against the per-sample-division form (host emulation of both) ------------------------------------------------
def _wave_incl_scan(v):
    """wave_incl_scan of csrc/ddsp_common.h on [..., 64] float64: row_shr 1, 2, 4, 8 inside the rows of 16, row_bcast15 onto rows 1 and
    3, row_bcast31 onto rows 2 and 3"""
    v = v.copy()
    lane = np.arange(64)
    for d in (1, 2, 4, 8):
        src = np.where((lane % 16) >= d, np.roll(v, d, axis=-1), 0.0)
        v = v + src
    add = np.zeros_like(v)
    add[..., 16:32] = v[..., 15:16]
    add[..., 48:64] = v[..., 47:48]
    v = v + add
    add = np.zeros_like(v)
    add[..., 32:64] = v[..., 31:32]
    return v + add


def _two_product(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp), float64 arrays"""
    def split(x):
        c = 134217729.0 * x
        hi = c - (c - x)
        return hi, x - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma64(a, b, c):
    """float64 fma(a, b, c), correctly rounded: the exact product as two float64 values, then an exact sum of three"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p, e = _two_product(a, b)
    out = np.array([math.fsum(t) for t in zip(p.reshape(-1).tolist(), e.reshape(-1).tolist(), c.reshape(-1).tolist())])
    return out.reshape(a.shape)


def _chunks(tot):
    F = tot.shape[0]
    chunk = (F + 255) // 256
    pad = np.zeros(256 * chunk)
    pad[:F] = tot
    return pad.reshape(256, chunk)


def _frame_prefix(tot, local_excl):
    """exclusive prefixes of the frame totals from the exclusive prefixes of the 256 chunk sums: the serial walk of a chunk"""
    ch = _chunks(tot)
    run = local_excl.copy()
    out = np.zeros_like(ch)
    for i in range(ch.shape[1]):
        out[:, i] = run
        run = run + ch[:, i]
    return out.reshape(-1)[:tot.shape[0]]


def _scan_hillis_steele(tot):
    local = np.zeros(256)
    for col in _chunks(tot).T:
        local = local + col
    part = local.copy()
    d = 1
    while d < 256:
        part = part + np.concatenate([np.zeros(d), part[:-d]])
        d <<= 1
    return _frame_prefix(tot, part - local)


def x_bits_both_forms(row, hop=512):
    """float32 x of one utterance (no initial phase) in the per-sample-division form and in the sum-first form"""
    F = row.shape[0]
    assert hop == 512
    v = upsample_f32(row, hop).astype(np.float64).reshape(F, 64, 8)
    rsr = 1.0 / SR
    # per-sample quotients (RN(v / sr): what PhaseCfg::term() returns)
    pre_q = np.cumsum(v / float(SR), axis=2)
    incl_q = _wave_incl_scan(pre_q[:, :, 7])
    base_q = _scan_hillis_steele(incl_q[:, 63])[:, None] + (incl_q - pre_q[:, :, 7])
    P = base_q[:, :, None] + pre_q
    x_old = (P - np.rint(P)).astype(np.float32)
    # sum first, scale once
    pre_s = np.cumsum(v, axis=2)
    incl_s = _wave_incl_scan(pre_s[:, :, 7])
    phase0 = _scan_hillis_steele(incl_s[:, 63] * rsr)
    base_s = _fma64(incl_s - pre_s[:, :, 7], rsr, phase0[:, None])
    P = _fma64(pre_s, rsr, base_s[:, :, None])
    x_new = (P - np.rint(P)).astype(np.float32)
    return x_old.reshape(-1), x_new.reshape(-1)


def test_bits_against_per_sample_division():
    """no kernel runs here: the two forms in float64 on the host, the counts of the module docstring (printed, and x held to 6e-8)"""
    rng = np.random.default_rng(77)
    front = np.exp(rng.uniform(np.log(100.0), np.log(800.0), (1, 17))).astype(np.float32)       # tests/test_front_same_bits.py
    counts = {}
    for name, rows in (("seed77_F17", front), ("mixed_F17", f0_rows("mixed", 17)), ("mixed_F257", f0_rows("mixed", 257))):
        n = differ = 0
        worst = 0.0
        for row in rows:
            a, b = x_bits_both_forms(row)
            d = a.astype(np.float64) - b
            worst = max(worst, float(np.abs(d - np.rint(d)).max()))
            differ += int((a.view(np.uint32) != b.view(np.uint32)).sum())
            n += a.size
        counts[name] = (differ, n)
        print("%s: %d of %d x values differ in their float32 bits, at most %.3g cycles" % (name, differ, n, worst))
        assert worst <= X_TOL
    assert counts["seed77_F17"][0] == 0                             # so tests/test_front_same_bits.py keeps its recorded signal


# ---- infer = False: nothing moves ---------------------------------------------------------------------------------------------------
NOINFER_F = (1, 17)


def compute_noinfer(dev):
    """phase0, x and a CombSub signal of the training path (infer=False), hop 512, B = 2 -- also what the generator records"""
    from ddsp_svc_amd import synth
    out = {}
    for F in NOINFER_F:
        rng = np.random.default_rng(300 + F)
        f0 = np.exp(rng.uniform(np.log(80.0), np.log(700.0), (2, F))).astype(np.float32)
        cg, ch, cn = (rng.standard_normal((2, F, 256)).astype(np.float32) for _ in range(3))
        u = rng.random((2, F * 512), dtype=np.float32)
        f0t, cgt, cht, cnt, ut = (torch.from_numpy(a).to(dev) for a in (f0, cg, ch, cn, u))
        ipt = torch.from_numpy(IP).to(dev)
        st = synth.phase(f0t, SR, 512, initial_phase=ipt, infer=False, want_x=True)
        sig, _, _ = synth.combsub_synth(f0t, st, cgt, cht, cnt, ut, SR, 512, noise_is_u01=True)
        out["phase0_%d" % F] = st.phase0.cpu().numpy().copy()
        out["x_%d" % F] = st.x.cpu().numpy().copy()
        out["signal_%d" % F] = sig.cpu().numpy().copy()
    return out


@pytest.mark.gpu
def test_noinfer_is_the_parent_bit_for_bit(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with np.load(os.path.join(golden_dir, NOINFER_FILE)) as z:
        recorded = {k: z[k] for k in z.files}
    got = compute_noinfer(torch.device("cuda:0"))
    assert sorted(got) == sorted(recorded)
    for key, a in got.items():
        b = recorded[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert np.isfinite(a).all(), key
        view = np.uint64 if a.dtype == np.float64 else np.uint32
        assert np.array_equal(a.view(view), b.view(view)), key
