"""f0 curves over the whole pitch range the reference's inference feeds the DSP, and the comparison bars the tests judge them by.

The extractors run with ``f0_min 50`` / ``f0_max 1100`` (main.py), clamp to ``f0_min`` after interpolating unvoiced frames
(ddsp/vocoder.py:139-143), and the key shift ``f0 * 2 ** (key / 12)`` (main.py:204; gui.py's pitch slider spans -24 .. +24)
then moves that band to 12.5 .. 4 400 Hz.  ``oracle.synth_f0`` stays inside 65 .. 800 Hz, so every regime here is built for
the parts of the kernels that depend on the SIZE of f0:

  glide          log glides 12.5 -> 4 400 Hz and back (every utterance its own direction and start)
  jumps          octave / two-octave jumps every few frames: 200 <-> 800, 100 <-> 1 600, 12.5 <-> 50 Hz (an extractor's
                 octave errors, a key change in the middle of a stream)
  nyquist        f0 with fl32(f0 k) == sr / 2 exactly for one harmonic k (the mask ``f0 k < sr / 2`` of core.py:75 is false
                 there and true one ulp below), mixed frame by frame with their float32 neighbours above and below, after
                 a lead-in at another pitch so that the harmonic at Nyquist does not sit on its zero crossings
  hw_edge        f0 whose CombSub half width fl32(1.5 sr / fl32(f0 + 1e-3)) (vocoder.py:851) is an integer or one ulp below
                 one (15, 41, 82, 255, ... and the powers of two): the tap at d = ceil(hw) is then at or next to the clamp
                 ``u > 1`` of core.py:245.  Only one ulp below a POWER OF TWO m does fl32(m / hw) round to exactly 1 (the
                 quotient is 1 + 2^-24, a tie to even; below any other integer the gap is wider than half an ulp of 1): there
                 the tap d = m is NOT clamped, the case ir_pfa.hip stage_window_row's ``dc + 1`` branch exists for
  floor_ceiling  12.5 Hz and 4 400 Hz held (the last utterance, if any, alternates between them every frame)

Everything is deterministic: numpy PCG64 streams from the seed, float32 searches for the exact values.
"""
import numpy as np

F32 = np.float32
SR, HOP = 44100, 512
LO, HI = 12.5, 4400.0
REGIMES = ("glide", "jumps", "nyquist", "hw_edge", "floor_ceiling")
# harmonics k with sr / 2 / k inside (or at the edge of) the reachable band; 2 and 3 lie above it (11 025 / 7 350 Hz)
NYQ_K = (2, 3, 5, 7, 10, 21, 50, 9, 14, 25, 63, 126, 128, 245)
HW_TARGETS = (15, 16, 32, 41, 64, 82, 128, 255, 256, 510, 512)


def nyquist_f0(k, sr=SR):
    """every float32 f with fl32(f k) == fl32(sr / 2), nearest ones first (there are one to three)"""
    nyq = F32(sr) / F32(2.0)
    kk = F32(k)
    f = F32(nyq / kk)
    cand = [f]
    lo = hi = f
    for _ in range(4):
        lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(np.inf))
        cand += [lo, hi]
    hits = [c for c in cand if F32(c * kk) == nyq]
    assert hits, k
    return sorted(hits, key=lambda c: abs(float(c) - float(nyq) / k))


def half_width(f0, sr=SR):
    """vocoder.py:851 in float32: 1.5 sr / (f0 + 1e-3)"""
    f0 = np.asarray(f0, F32)
    return (F32(1.5) * F32(sr) / (f0 + F32(1e-3)).astype(F32)).astype(F32)


def hw_edge_f0(m, sr=SR, below=True):
    """a float32 f0 whose half width is exactly ``m`` (``below=False``) or the float32 just below ``m``; None if no f0
    rounds there (searched over the float32 neighbourhood of 1.5 sr / m - 1e-3)"""
    target = np.nextafter(F32(m), F32(0)) if below else F32(m)
    f = F32(F32(1.5) * F32(sr) / F32(m) - F32(1e-3))
    fs = [f]
    a = b = f
    for _ in range(64):
        a, b = np.nextafter(a, F32(0)), np.nextafter(b, F32(np.inf))
        fs += [a, b]
    fs = np.array(fs, F32)
    hit = fs[half_width(fs, sr) == target]
    return None if hit.size == 0 else F32(hit[np.argmin(np.abs(hit.astype(np.float64) - float(f)))])


def hw_edge_values(sr=SR):
    """(f0, hw) pairs of the hw_edge regime: hw one ulp below an integer where such an f0 exists, else the integer itself"""
    out = []
    for m in HW_TARGETS:
        for below in (True, False):
            f = hw_edge_f0(m, sr, below)
            if f is not None:
                out.append((f, half_width(f, sr)))
    assert out
    return out


def pitch_f0(regime, B, F, seed=0, sr=SR, lo=LO, hi=HI):
    """``[B, F, 1]`` float32 f0 of one regime (see the module docstring)"""
    rng = np.random.default_rng(seed)
    f0 = np.empty((B, F), np.float64)
    if regime == "glide":
        for b in range(B):
            t = np.linspace(0.0, 2.0, F) + rng.uniform(0.0, 0.5)
            tri = 1.0 - np.abs(1.0 - np.mod(t, 2.0))                   # 0 -> 1 -> 0
            if b % 2:
                tri = 1.0 - tri                                         # 4 400 -> 12.5 -> 4 400
            f0[b] = lo * (hi / lo) ** tri
    elif regime == "jumps":
        pairs = ((200.0, 800.0), (100.0, 1600.0), (12.5, 50.0))
        for b in range(B):
            a, c = pairs[b % 3]
            run = 2 + (b % 3)
            up = (np.arange(F) // run) % 2 == 1
            f0[b] = np.where(up, c, a) * 2.0 ** (rng.normal(0.0, 0.05, F) / 12.0)
    elif regime == "nyquist":
        ks = list(NYQ_K)
        for b in range(B):
            k = ks[int(rng.integers(len(ks)))] if b else 21
            exact = nyquist_f0(k, sr)[0]
            choices = np.array([exact, np.nextafter(exact, F32(0)), np.nextafter(exact, F32(np.inf))], F32)
            pick = rng.integers(0, 3, F)
            pick[: F // 4] = 0                                         # a run of the exact value (masked in both frames of a hop)
            row = choices[pick].astype(np.float64)
            lead = min(3, F - 1)
            row[:lead] = float(exact) * 0.83                            # lead-in: the phase of harmonic k is not on its zeros
            f0[b] = row
    elif regime == "hw_edge":
        vals = np.array([f for f, _ in hw_edge_values(sr)], F32)
        for b in range(B):
            f0[b] = vals[rng.integers(0, vals.size, F)]
    elif regime == "floor_ceiling":
        for b in range(B):
            f0[b] = (lo, hi)[b % 2] if b < 2 else np.where(np.arange(F) % 2 == 0, lo, hi)
    else:
        raise ValueError(regime)
    out = f0.astype(F32)
    if regime in ("glide", "jumps", "floor_ceiling"):
        out = np.clip(out, F32(lo), F32(hi)) if regime != "jumps" else out
    return out[:, :, None]


CTRL_KINDS = ("unit", "wide", "quiet")


def pitch_controls(B, F, sizes, kind="unit", seed=0, noise_index=-1):
    """raw control streams ``[B, F, n]`` float32: ``unit`` N(0, 1); ``wide`` sigma = 3; ``quiet`` N(0, 1) except the noise
    band's control (``sizes[noise_index]``, None: none), whose mean is -5 -- the noise part is then ~1 / 150 of its usual
    level, and the harmonic part is judged separately anyway"""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        c = rng.standard_normal((B, F, n))
        if kind == "wide":
            c = 3.0 * c
        elif kind == "quiet" and noise_index is not None and i == (noise_index % len(sizes)):
            c = c - 5.0
        out.append(c.astype(F32))
    return out


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


# the two bars of the pitch-range tests, fixed before any run on the hardware: the fuzz tests' whole-utterance bar, and a per-hop
# bar that a single harmonic wrongly masked or unmasked in one hop (1e-2 .. 1e-1 of the component) cannot pass
UTT_BAR = 2e-5
HOP_BAR = 1e-4


def judge(got, ref, hop=HOP, what=""):
    """-> (worst whole-utterance relative RMS, worst per-hop RMS relative to its utterance's RMS); asserts both bars.
    ``got`` / ``ref`` are ``[B, T]``; a silent utterance (RMS 0) is judged against 1e-9."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    B, T = ref.shape
    worst_u = worst_h = 0.0
    for b in range(B):
        r = max(rms(ref[b]), 1e-9)
        d = got[b] - ref[b]
        eu = rms(d) / r
        nh = T // hop
        eh = float(np.sqrt(np.mean(np.square(d[: nh * hop].reshape(nh, hop)), axis=1)).max()) / r if nh else 0.0
        worst_u, worst_h = max(worst_u, eu), max(worst_h, eh)
        assert eu <= UTT_BAR, (what, b, "utterance", eu)
        assert eh <= HOP_BAR, (what, b, "hop", eh, int(np.argmax(np.sqrt(np.mean(np.square(d[: nh * hop].reshape(nh, hop)), axis=1)))))
    return worst_u, worst_h


# ---- the reference fixtures pitch_*.npz (tests/golden/make_golden.py --pitch-range): inputs regenerated from these seeds ----
PITCH_DEC = 7       # waveforms are stored every 7th sample (prime: the stored samples walk through every position in a hop)
PITCH_F = 24
PITCH_SETS = {"a": (("glide", 0), ("jumps", 1), ("nyquist", 0)), "b": (("hw_edge", 0), ("floor_ceiling", 1), ("jumps", 2))}
PITCH_TAILS = {"sins": (256, 256, 129), "combsub": (256, 256, 256), "csfast": (513, 513, 513), "cssuper": (1025,) * 4}
PITCH_SIZES_B = {"combsub": (257, 512, 129)}          # CombSub's b fixture: the chirp-z tap forms


def pitch_inputs(tag, kind, sr=SR, hop=HOP):
    """``(f0 [3, 24, 1], sizes, controls, noise)`` of pitch_{kind}_{tag}.npz: a (glide, 100 <-> 1 600 Hz jumps, Nyquist k = 21;
    controls N(0, 1)), b (hw_edge, 4 400 Hz held, 12.5 <-> 50 Hz jumps; controls sigma 3).  ``noise`` is the uniform(-1, 1)
    draw, for cssuper the standard-normal one."""
    from oracle import ddsp_oracle as O
    f0 = np.stack([pitch_f0(reg, 3, PITCH_F, seed=1)[r] for reg, r in PITCH_SETS[tag]]).astype(F32)
    sizes = PITCH_SIZES_B.get(kind, PITCH_TAILS[kind]) if tag == "b" else PITCH_TAILS[kind]
    seed = 7000 + 10 * list(PITCH_TAILS).index(kind) + (tag == "b")
    ctrls = pitch_controls(3, PITCH_F, sizes, "unit" if tag == "a" else "wide", seed=seed)
    if kind == "cssuper":
        noise = O.synth_gauss(3, PITCH_F * hop, seed=seed + 1)
    else:
        noise = O.synth_noise(3, PITCH_F * hop, seed=seed + 1)
    return f0, sizes, ctrls, noise


def input_checks(a):
    """the identifying numbers make_golden.py stores for a regenerated input (sum, sum of squares, a few values)"""
    a = np.asarray(a, np.float64).reshape(-1)
    return np.array([a.sum(), np.square(a).sum(), a[0], a[1], a[a.size // 2], a[-1]], np.float64)


def sins_skipped_bank(x, f0_frames, c_amp, sr=SR, hop=HOP):
    """The part of ``O.sinusoid_bank`` the hop-512 Sins kernel leaves out by design (exciter.hip k_sins_bank3, knob SINS_NOSKIP = 0,
    the default): per hop, the trailing blocks of 17 harmonics whose lowest harmonic is at or above Nyquist in BOTH frames, and the
    one or two harmonics past the last whole block when a block was dropped or they are masked in both frames.  Those harmonics
    carry 1e-7 of their amplitude (core.py:75-76); in range that is < 3e-7 of the exciter (tests/test_parity.py
    test_sinusoid_bank), but with sigma = 3 controls and f0 so high that one or two harmonics survive, the 1e-7 of the strongest
    masked ones reaches 2e-5 of the utterance (float64 evidence: Nyquist regime, k = 2, f0 = 11 025 Hz: kernel 2.2e-5 from the
    oracle with the skip, 3.8e-7 with SINS_NOSKIP = 1, and 2.2e-5 is what this function returns).  Returns ``[B, T]`` float64."""
    c_amp = np.asarray(c_amp, F32)
    f0 = np.asarray(f0_frames, F32).reshape(c_amp.shape[0], -1)
    B, Fr, H = c_amp.shape
    W = 17
    rem = H % W
    nblk_all = H // W + (1 if rem > 2 else 0)
    nsingle_all = 0 if rem > 2 else rem
    nyq = F32(sr) / F32(2.0)
    skipped = np.zeros((B, Fr, H), bool)
    for b in range(B):
        for f in range(Fr):
            fa, fb = f0[b, f], f0[b, min(f + 1, Fr - 1)]
            masked = lambda k: F32(fa * F32(k)) >= nyq and F32(fb * F32(k)) >= nyq
            nblk = nblk_all
            while nblk > 0 and masked(1 + W * (nblk - 1)):
                nblk -= 1
            nsingle = nsingle_all if nblk == nblk_all else 0
            while nsingle > 0 and masked(W * nblk_all + nsingle):
                nsingle -= 1
            keep = np.zeros(H, bool)
            keep[: min(W * nblk, H)] = True
            keep[W * nblk_all: W * nblk_all + nsingle] = True
            skipped[b, f] = ~keep
    from oracle import ddsp_oracle as O
    A = (np.exp(c_amp.astype(np.float64)) / 128.0).astype(F32)
    A = O.remove_above_fmax(A, f0, nyq, 1)
    phase = (O.TWO_PI32 * np.asarray(x, F32)).astype(F32)
    out = np.zeros(phase.shape, np.float64)
    ks = np.arange(1, H + 1, dtype=F32)
    for h0 in range(0, H, 16):
        sk = skipped[:, :, h0:h0 + 16]
        if not sk.any():
            continue
        arg = (phase[:, :, None] * ks[None, None, h0:h0 + 16]).astype(F32)
        amp = O.upsample(A[:, :, h0:h0 + 16], hop).astype(np.float64) * np.repeat(sk, hop, axis=1)
        out += (np.sin(arg.astype(np.float64)) * amp).sum(-1)
    return out
