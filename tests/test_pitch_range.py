"""The synthesisers across the pitch range key shifting reaches: 12.5 .. 4 400 Hz (tests/pitch_regimes.py).

Every other synthesis test draws f0 from 65 .. 800 Hz.  The reference's inference feeds the DSP f0_min 50 .. f0_max 1100 Hz times
2 ** (key / 12) with key in -24 .. +24 (main.py:204, gui.py:109, :240), and several kernel paths depend on how large f0 is: the
dynamic window built from ``hw = 1.5 sr / (f0 + 1e-3)`` in the three tap-synthesis forms (its clamp threshold, a cosine angle that
grows as 255 / hw), the exciter's ``sinc`` (arguments up to pi sr / (2 f0) = 5 541 rad), the Sins Nyquist mask and the skip of
masked harmonic blocks (an exact ``f0 k == sr / 2``, a harmonic masked in one frame and not the next), the NSF source's harmonics
above Nyquist.

Bars (fixed before any hardware run):
  tails              relative RMS <= 2e-5 per utterance (test_fuzz.py's bar) AND, for every hop, error RMS <= 1e-4 of the
                     utterance's RMS of that component (a single wrongly masked harmonic in one hop is 1e-2 .. 1e-1 of it)
  combtooth          max abs <= 1e-6 per sample (sine 3.9e-7 abs / |p| >= 2, Taylor branch 1.2e-8, one ulp of z from div_pos:
                     <= 3e-7 in all)
  sinusoid bank      the tails' two bars, hop by hop
  NSF source         max abs <= 2e-6 (test_sine_source_shapes)
  adjoints           relative RMS <= 1e-5 (sinusoid bank, test_fuzz.py) / 2e-5 (CombSub tail, test_fused_tail_training_node)
Emulator shapes stay at B <= 3, F <= 48; the shape above kSmallRows = 4096 frames runs on the GPU only.
"""
import os

import numpy as np
import pytest
import torch

from oracle import ddsp_oracle as O
from tests import pitch_regimes as P
from tests.backends import BACKENDS, dev  # noqa: F401

SR, HOP = 44100, 512
REGIMES = P.REGIMES
rms = P.rms


def T_(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def N_(t):
    return t.detach().cpu().numpy()


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _fixture_inputs(g, tag, kind):
    """the regenerated inputs of a pitch_*.npz fixture, refused if they are not the numbers the reference ran on"""
    f0, sizes, ctrls, noise = P.pitch_inputs(tag, kind)
    assert np.array_equal(f0, g["f0_frames"]) and tuple(g["sizes"]) == tuple(sizes)
    assert np.allclose(P.input_checks(noise), g["noise_check"], rtol=1e-12, atol=0)
    checks = sorted(k for k in g.files if k.startswith("check_"))
    assert len(checks) == len(ctrls)
    return f0, sizes, ctrls, noise


NAMES = {"sins": ("amplitudes", "group_delay", "noise_magnitude"),
         "combsub": ("group_delay", "harmonic_magnitude", "noise_magnitude"),
         "csfast": ("harmonic_magnitude", "harmonic_phase", "noise_magnitude"),
         "cssuper": ("harmonic_magnitude", "harmonic_phase", "noise_magnitude", "noise_phase")}


def _check_ctrls(g, kind, ctrls):
    for k, c in zip(NAMES[kind], ctrls):
        assert np.allclose(P.input_checks(c), g["check_" + k], rtol=1e-12, atol=0), k


def _oracle(kind, f0, ctrls, noise, sins_skip=True):
    """the oracle's tail; for Sins with the kernel's skip of masked harmonic blocks (``sins_skip``, the default knob setting)
    minus exactly what that skip leaves out (P.sins_skipped_bank, through the same linear all-pass filter)"""
    if kind == "sins":
        r = O.sins_dsp(f0, *ctrls, noise, SR, HOP)
        if sins_skip:
            left_out = O.frequency_filter(P.sins_skipped_bank(r["x"], f0, ctrls[0], SR, HOP), *O.allpass_response(ctrls[1]), O.MODE_ROLL)
            r = dict(r, signal=r["signal"] - left_out, harmonic=r["harmonic"] - left_out)
        return r
    if kind == "combsub":
        return O.combsub_dsp(f0, *ctrls, noise, SR, HOP)
    if kind == "csfast":
        return O.combsubfast_dsp(f0, *ctrls, noise, SR, HOP)
    return O.combsubsuperfast_dsp(f0, *ctrls, noise, SR, HOP)


# ================================================================================================================================
# 1. the oracle against the reference at the extended range (CPU)
# ================================================================================================================================
@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("kind", ["sins", "combsub", "csfast", "cssuper"])
def test_oracle_pitch_range_golden(golden_dir, kind, tag):
    """the oracle's tails against the reference's own forward at 12.5 .. 4 400 Hz (pitch_{kind}_{tag}.npz); bars of
    test_oracle_golden.py (5e-6 for Sins / CombSub, whose float32 pipeline sits ~1.5e-6 from float64; 2e-6 for the spectral
    tails), on the stored every-7th samples, per component"""
    g = _load(golden_dir, f"pitch_{kind}_{tag}.npz")
    f0, _, ctrls, noise = _fixture_inputs(g, tag, kind)
    _check_ctrls(g, kind, ctrls)
    r = _oracle(kind, f0, ctrls, noise, sins_skip=False)
    dec = int(g["dec"])
    keys = (("signal", "signal"), ("harmonic", "harmonic"), ("noise", "noise_out")) if kind in ("sins", "combsub") else (("signal", "signal"),)
    bar = 5e-6 if kind in ("sins", "combsub") else 2e-6
    for k, gk in keys:
        got = r[k][:, ::dec]
        for b in range(got.shape[0]):
            e, s = rms(got[b] - g[gk][b]), rms(g[gk][b])
            assert e <= bar * s, (kind, tag, k, b, e, s)
    if kind in ("csfast", "cssuper"):
        assert np.array_equal(r["phase_frames"], g["phase_frames"])


def test_oracle_pitch_range_fast_source(golden_dir):
    """CombSubSuperFast.fast_source_gen at 12.5 .. 4 400 Hz: the float32 phase recipe bit for bit, the exciter (its sinc argument
    reaches pi sr / (2 f0) = 5 541 rad at 12.5 Hz) within 2e-7 of the reference's float32 sinc"""
    g = _load(golden_dir, "pitch_fastsrc.npz")
    comb, pf, _ = O.fast_source_gen(g["f0_frames"], SR, HOP)
    assert np.array_equal(pf, g["phase_frames"])
    assert np.abs(comb[:, ::int(g["dec"])] - g["combtooth"]).max() <= 2e-7


def test_oracle_pitch_range_sine_source(golden_dir):
    """SourceModuleHnNSF, dim 9, at f0 up to 4 400 Hz (harmonics above Nyquist from 2 450 Hz) with unvoiced frames"""
    g = _load(golden_dir, "pitch_sinesrc.npz")
    f0 = g["f0"]
    nz = np.random.default_rng(int(g["noise_seed"])).standard_normal((f0.shape[0], f0.shape[1] * HOP, 9)).astype(np.float32)
    assert np.allclose(P.input_checks(nz), g["noise_check"], rtol=1e-12, atol=0)
    out = O.sine_source(f0, HOP, SR, g["weight"], g["bias"], g["rand_ini"], nz)
    assert np.abs(out[:, ::int(g["dec"])] - g["out"]).max() <= 2e-6


def test_window_clamp_threshold_is_floor_plus_one():
    """The dynamic window clamps ``u = fl32(d / hw) > 1`` (core.py:245); the kernels clamp ``d >= thr`` with thr from
    ir_pfa.hip stage_window_row: floor(hw) + 1, or one more where fl32((floor(hw) + 1) / hw) rounds to exactly 1.  It never
    does: for hw < m (m = floor(hw) + 1) the quotient exceeds 1 by more than ulp(hw) / m >= 2^-24 and rounds up, so that second
    branch cannot be taken and thr = floor(hw) + 1 is the reference's clamp for EVERY float32 half width in [0.5, 1024) -- checked
    here exhaustively (92 274 688 values).  (A test cannot tell the branch from its absence; this one pins why.)"""
    lo, hi = int(np.float32(0.5).view(np.int32)), int(np.float32(1024).view(np.int32))
    for s in range(lo, hi, 1 << 22):
        hw = np.arange(s, min(s + (1 << 22), hi), dtype=np.int64).astype(np.int32).view(np.float32)
        m = np.floor(hw) + np.float32(1)
        assert (m / hw > np.float32(1)).all() and (np.floor(hw) / hw <= np.float32(1)).all()


def test_regimes_hit_their_edges():
    """the generator does what the tests rely on: exact fl32(f0 k) == sr / 2 frames next to unmasked neighbours, half widths on and
    one ulp below integers, the floor and the ceiling, deterministic"""
    nyq = np.float32(SR / 2)
    f0 = P.pitch_f0("nyquist", 3, 40, seed=1)[..., 0]
    assert np.array_equal(f0, P.pitch_f0("nyquist", 3, 40, seed=1)[..., 0])
    exact = P.nyquist_f0(21)[0]
    assert (f0[0] == exact).sum() >= 10 and (f0[0] < exact).any() and (f0[0] > exact).any()
    assert np.float32(exact * np.float32(21)) == nyq and np.float32(np.nextafter(exact, np.float32(0)) * np.float32(21)) < nyq
    hws = [hw for _, hw in P.hw_edge_values()]
    assert {15.0, 41.0, 82.0} <= {float(h) for h in hws} and any(hw != np.floor(hw) for hw in hws)
    fc = P.pitch_f0("floor_ceiling", 3, 8)[..., 0]
    assert fc.min() == np.float32(12.5) and fc.max() == np.float32(4400)
    gl = P.pitch_f0("glide", 2, 48, seed=3)[..., 0]
    assert gl.min() < 20 and gl.max() > 3000
    j = P.pitch_f0("jumps", 3, 12, seed=3)[..., 0]
    assert (np.abs(np.diff(np.log2(j), axis=1)) > 0.9).sum(axis=1).min() >= 2


# ================================================================================================================================
# 2. forward parity, the four functional tails, every regime
# ================================================================================================================================
def _run_tail(kind, dev, f0, ctrls, noise):
    from ddsp_svc_amd import synth
    t = lambda a: T_(a, dev)
    if kind == "sins":
        st = synth.phase(t(f0), SR, HOP)
        out = synth.sins_synth(t(f0), st, *[t(c) for c in ctrls], t(noise), SR, HOP)
        return dict(zip(("signal", "harmonic", "noise"), (N_(o) for o in out)))
    if kind == "combsub":
        st = synth.phase(t(f0), SR, HOP)
        out = synth.combsub_synth(t(f0), st, *[t(c) for c in ctrls], t(noise), SR, HOP)
        return dict(zip(("signal", "harmonic", "noise"), (N_(o) for o in out)))
    if kind == "csfast":
        st = synth.phase(t(f0), SR, HOP)
        w = torch.sqrt(torch.hann_window(1024)).to(dev)
        return {"signal": N_(synth.combsubfast_synth(t(f0), st, *[t(c) for c in ctrls], t(noise), w, SR, HOP))}
    st = synth.fast_source(t(f0), SR, HOP)
    w = torch.hann_window(2048).to(dev)
    return {"signal": N_(synth.combsubsuperfast_synth(t(f0), st, *[t(c) for c in ctrls], t(noise), w, SR, HOP))}


def _inputs(kind, B, F, f0_seed_regime, ctrl_kind, seed, sizes=None):
    sizes = sizes or {"sins": (256, 256, 256), "combsub": (256, 256, 256), "csfast": (513,) * 3, "cssuper": (1025,) * 4}[kind]
    ctrls = P.pitch_controls(B, F, sizes, ctrl_kind, seed=seed, noise_index=2)
    noise = O.synth_gauss(B, F * HOP, seed=seed + 1) if kind == "cssuper" else O.synth_noise(B, F * HOP, seed=seed + 1)
    return ctrls, noise


def _compare(kind, got, ref, what):
    worst = {}
    for k in got:
        worst[k] = P.judge(got[k], ref[k], HOP, what=(kind,) + tuple(what) + (k,))
    return worst


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("ctrl_kind", P.CTRL_KINDS)
@pytest.mark.parametrize("regime", REGIMES)
def test_tails_across_pitch_regimes(dev, regime, ctrl_kind):
    """Sins / CombSub (signal, harmonic, noise) and CombSubFast / CombSubSuperFast (signal) against the oracle, every regime, three
    control scales, per utterance and per hop"""
    B, F = 3, 40
    f0 = P.pitch_f0(regime, B, F, seed=11)
    for i, kind in enumerate(("sins", "combsub", "csfast", "cssuper")):
        ctrls, noise = _inputs(kind, B, F, regime, ctrl_kind, seed=100 * i + len(regime))
        _compare(kind, _run_tail(kind, dev, f0, ctrls, noise), _oracle(kind, f0, ctrls, noise), (regime, ctrl_kind))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("setting", [("SMALL_PATH", 1), ("SINS_NOSKIP", 0), ("SINS_NOSKIP", 1), ("BLK_RUN", 3), ("TAPS_GEMM", 1)])
@pytest.mark.parametrize("regime", ["nyquist", "jumps", "hw_edge", "glide"])
def test_tails_under_knobs(dev, regime, setting, knobs):
    """the same comparison with the launcher's alternatives forced: the batch layout at a streaming shape (SMALL_PATH = 1), the
    Sins bank with and without the skip of masked blocks (each against the oracle: with the skip, minus what it leaves out by
    design), a run split of the hop-block filter, the dense tap contraction at 256 bins"""
    knobs(*setting)
    B, F = 3, 33
    f0 = P.pitch_f0(regime, B, F, seed=12)
    for i, kind in enumerate(("sins", "combsub")):
        ctrls, noise = _inputs(kind, B, F, regime, "unit", seed=300 + i)
        ref = _oracle(kind, f0, ctrls, noise, sins_skip=setting != ("SINS_NOSKIP", 1))
        _compare(kind, _run_tail(kind, dev, f0, ctrls, noise), ref, (regime,) + setting)
    if setting == ("SINS_NOSKIP", 1):                          # every harmonic evaluated: the full oracle, wide controls too
        ctrls, noise = _inputs("sins", B, F, regime, "wide", seed=302)
        _compare("sins", _run_tail("sins", dev, f0, ctrls, noise), _oracle("sins", f0, ctrls, noise, sins_skip=False), (regime, "wide") + setting)
    if setting[0] == "SMALL_PATH":
        ctrls, noise = _inputs("cssuper", B, F, regime, "unit", seed=310)
        _compare("cssuper", _run_tail("cssuper", dev, f0, ctrls, noise), _oracle("cssuper", f0, ctrls, noise), (regime,) + setting)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("sr", [44100, 32000])
@pytest.mark.parametrize("n", [256, 512, 129, 200, 65])
@pytest.mark.parametrize("regime", ["hw_edge", "glide", "floor_ceiling"])
def test_combsub_window_forms(dev, regime, n, sr):
    """CombSub's harmonic filter at bin counts that reach each tap-synthesis form (api.hip synth_taps): 256 the prime-factor form,
    512 / 129 / 200 the chirp-z form, 65 the dense contraction -- each builds the f0-derived window itself; at 32 kHz the hw_edge
    regime has half widths one ulp below 16 .. 512, where the clamp's threshold is one tap further out"""
    B, F = 2, 24
    f0 = P.pitch_f0(regime, B, F, seed=13, sr=sr)
    ctrls, noise = _inputs("combsub", B, F, regime, "unit", seed=400 + n, sizes=(n, n, n))
    from ddsp_svc_amd import synth
    t = lambda a: T_(a, dev)
    st = synth.phase(t(f0), sr, HOP)
    out = synth.combsub_synth(t(f0), st, *[t(c) for c in ctrls], t(noise), sr, HOP)
    got = dict(zip(("signal", "harmonic", "noise"), (N_(o) for o in out)))
    _compare("combsub", got, O.combsub_dsp(f0, *ctrls, noise, sr, HOP), (regime, n, sr))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("n", [256, 512, 129, 65])
def test_dynamic_window_at_the_clamp(dev, n):
    """the dynamic-window taps (MagnitudeTapsFunction, the training path's synthesis) for half widths on, and one and two ulps below,
    integers from 15 (f0 = 4 410 Hz) up to the last tap, and 1e4 (f0 below 7 Hz: nothing clamped), against the oracle's
    float32 window: per row 2e-6"""
    from ddsp_svc_amd import synth
    N = 2 * (n - 1)
    ms = [m for m in (15, 16, 32, 41, 64, 82, 128, 255, 256, 510, 512) if m < N // 2]
    hw = []
    for m in ms:
        a = np.float32(m)
        hw += [a, np.nextafter(a, np.float32(0)), np.nextafter(np.nextafter(a, np.float32(0)), np.float32(0))]
    hw += [np.float32(1e4)]
    hw = np.array(hw, np.float32).reshape(1, -1)
    F = hw.shape[1]
    (c,) = P.pitch_controls(1, F, [n], "unit", seed=29)
    taps = N_(synth.MagnitudeTapsFunction.apply(T_(c, dev), 1.0, O.MODE_DYNAMIC, T_(hw, dev)))
    ref = O.impulse_response(np.exp(c.astype(np.float64)), None, O.MODE_DYNAMIC, hw)
    for f in range(F):
        e, r = rms(taps[0, f] - ref[0, f]), rms(ref[0, f])
        assert e <= 2e-6 * r, (n, float(hw[0, f]), e, r)


@pytest.mark.gpu
@pytest.mark.parametrize("dev", ["gpu"], indirect=True)
@pytest.mark.parametrize("kind", ["sins", "combsub", "cssuper"])
def test_tails_batch_shape_gpu(dev, kind):
    """the batch layout above kSmallRows = 4 096 frames (5 x 840 rows), all five regimes stacked per utterance"""
    B, F = 5, 840
    f0 = np.concatenate([P.pitch_f0(r, 1, F, seed=14 + i) for i, r in enumerate(REGIMES)]).astype(np.float32)
    sizes = {"sins": (128, 256, 256), "combsub": (256, 256, 256), "cssuper": (1025,) * 4}[kind]
    ctrls, noise = _inputs(kind, B, F, "mixed", "unit", seed=500, sizes=sizes)
    _compare(kind, _run_tail(kind, dev, f0, ctrls, noise), _oracle(kind, f0, ctrls, noise), ("batch",))


# ================================================================================================================================
# 3. the drop-in modules and the streaming sessions
# ================================================================================================================================
class FixedUnit2Control(torch.nn.Module):
    """Unit2Control's interface returning the controls it was given, as split views of one tensor (as the real one does)"""

    def __init__(self, n_unit, n_spk, output_splits, **kwargs):
        super().__init__()
        self.output_splits = output_splits
        self.ctrls = None

    def forward(self, units, f0, phase, volume, spk_id=None, spk_mix_dict=None, aug_shift=None):
        whole = torch.cat(self.ctrls, -1)
        return dict(zip(self.output_splits, torch.split(whole, list(self.output_splits.values()), -1))), units


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("kind", ["sins", "combsub", "csfast", "cssuper"])
@pytest.mark.parametrize("regime", ["jumps", "nyquist", "floor_ceiling"])
def test_modules_across_pitch_regimes(dev, regime, kind, monkeypatch):
    """vocoder.Sins / CombSub / CombSubFast / CombSubSuperFast.forward with fixed controls and injected draws"""
    from ddsp_svc_amd import vocoder as V
    B, F = 2, 20
    f0 = P.pitch_f0(regime, B, F, seed=15)
    sizes = {"sins": (256, 256, 129), "combsub": (256, 256, 256), "csfast": (513,) * 3, "cssuper": (1025,) * 4}[kind]
    ctrls, noise = _inputs(kind, B, F, regime, "unit", seed=600, sizes=sizes)
    if kind == "sins":
        m = V.Sins(SR, HOP, *sizes, n_unit=4, unit2ctrl_factory=FixedUnit2Control)
    elif kind == "combsub":
        m = V.CombSub(SR, HOP, *sizes, n_unit=4, unit2ctrl_factory=FixedUnit2Control)
    elif kind == "csfast":
        m = V.CombSubFast(SR, HOP, n_unit=4, unit2ctrl_factory=FixedUnit2Control)
    else:
        m = V.CombSubSuperFast(SR, HOP, 2048, n_unit=4, unit2ctrl_factory=FixedUnit2Control)
    m = m.to(dev).eval()
    m.unit2ctrl.ctrls = [T_(c, dev) for c in ctrls]
    if kind == "cssuper":
        monkeypatch.setattr(torch, "randn", lambda *a, **k: T_(noise, dev))
    else:
        u01 = ((noise + np.float32(1)) / np.float32(2)).astype(np.float32)
        assert np.array_equal((u01 * np.float32(2) - np.float32(1)).astype(np.float32), noise)
        monkeypatch.setattr(torch, "rand", lambda *a, **k: T_(u01, dev))
    with torch.no_grad():
        signal, _, (h, n) = m(torch.zeros(B, F, 4, device=dev), T_(f0, dev), torch.zeros(B, F, 1, device=dev))
    got = {"signal": N_(signal)}
    if kind in ("sins", "combsub"):
        got.update(harmonic=N_(h), noise=N_(n))
    _compare(kind, got, _oracle(kind, f0, ctrls, noise), ("module", regime))


def _key_change_f0(B, F, seed, key):
    """an f0 curve in the extractor's 50 .. 1 100 Hz band, shifted by ``key`` semitones from frame F / 2 on (gui.py's slider)"""
    f0 = P.pitch_f0("glide", B, F, seed=seed, lo=50.0, hi=1100.0)[..., 0].astype(np.float64)
    f0[:, F // 2:] *= 2.0 ** (key / 12.0)
    return f0.astype(np.float32)[:, :, None]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_superfast_streaming_key_change(dev):
    """synth.StreamingCombSubSuperFast (the model gui.py runs) through a stream whose key jumps +24 and then -24 semitones
    halfway through a call: every call the functional API's bits, and the oracle within the bars"""
    from ddsp_svc_amd import synth
    B, F, n = 1, 47, 1025
    w = torch.hann_window(2048).to(dev)
    sess = synth.StreamingCombSubSuperFast(B, F, w, SR, HOP, dev)
    for call, key in enumerate((0, 24, -24, 24)):
        f0 = _key_change_f0(B, F, seed=call, key=key)
        ctrls, noise = _inputs("cssuper", B, F, "stream", "unit", seed=700 + call)
        a = [T_(x, dev) for x in (f0, *ctrls, noise)]
        fs = synth.fast_source(a[0], SR, HOP)
        want = synth.combsubsuperfast_synth(a[0], fs, *a[1:5], a[5], w, SR, HOP)
        st = sess.source(a[0])
        assert torch.equal(st.rad_acc, fs.rad_acc) and torch.equal(st.phase_frames, fs.phase_frames)
        got = sess.synth(a[0], *a[1:5], a[5])
        assert torch.equal(got, want), (call, key)
        P.judge(N_(got), O.combsubsuperfast_dsp(f0, *ctrls, noise, SR, HOP)["signal"], what=("stream", call, key))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_combsub_streaming_key_change(dev):
    """synth.StreamingCombSub through the same stream: the functional API's bits (all three outputs), and the oracle"""
    from ddsp_svc_amd import synth
    B, F, n = 1, 43, 256
    sess = synth.StreamingCombSub(B, F, n, n, n, SR, HOP, dev, want_components=True)
    for call, key in enumerate((0, -24, 24)):
        f0 = _key_change_f0(B, F, seed=10 + call, key=key)
        ctrls, noise = _inputs("combsub", B, F, "stream", "unit", seed=800 + call)
        a = [T_(x, dev) for x in (f0, *ctrls, noise)]
        st = synth.phase(a[0], SR, HOP)
        want = synth.combsub_synth(a[0], st, *a[1:4], a[4], SR, HOP)
        ss = sess.phase(a[0])
        assert torch.equal(ss.phase_frames, st.phase_frames)
        got = sess.synth(a[0], *a[1:4], a[4])
        ref = O.combsub_dsp(f0, *ctrls, noise, SR, HOP)
        for g_, w_, k in zip(got, want, ("signal", "harmonic", "noise")):
            assert torch.equal(g_, w_), (call, key, k)
            P.judge(N_(g_), ref[k], what=("stream", call, key, k))


# ================================================================================================================================
# 4. against the reference's fixtures (both backends)
# ================================================================================================================================
@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("kind", ["sins", "combsub", "csfast", "cssuper"])
def test_tails_against_pitch_range_golden(dev, golden_dir, kind, tag):
    """the kernels against the reference's own output at 12.5 .. 4 400 Hz, on the stored samples: 1e-5 relative per utterance (the
    reference's float32 pipeline is itself ~1.5e-6 .. 5e-6 from float64)"""
    g = _load(golden_dir, f"pitch_{kind}_{tag}.npz")
    f0, _, ctrls, noise = _fixture_inputs(g, tag, kind)
    got = _run_tail(kind, dev, f0, ctrls, noise)
    dec = int(g["dec"])
    for k, gk in (("signal", "signal"), ("harmonic", "harmonic"), ("noise", "noise_out")):
        if k not in got:
            continue
        for b in range(3):
            e, s = rms(got[k][b, ::dec] - g[gk][b]), rms(g[gk][b])
            assert e <= 1e-5 * s, (kind, tag, k, b, e, s)


# ================================================================================================================================
# 5. primitives at the new argument ranges
# ================================================================================================================================
@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("regime", REGIMES)
def test_combtooth_full_range(dev, regime):
    """synth.combtooth (sinc(sr x / (f0 + 1e-3)), arguments up to 5 541 rad) against the float64 sine of the same float32
    argument: max abs 1e-6 per sample"""
    from ddsp_svc_amd import synth
    f0 = P.pitch_f0(regime, 3, 40, seed=16)
    st = synth.phase(T_(f0, dev), SR, HOP)
    out = N_(synth.combtooth(T_(f0, dev), st, SR, HOP))
    x, _ = O.wrapped_phase(f0, SR, HOP)
    ref = O.combtooth(x, f0, SR, HOP)
    err = np.abs(out - ref).max()
    assert err <= 1e-6, (regime, err)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("regime", REGIMES)
def test_fast_source_full_range(dev, regime):
    """synth.fast_source(want_combtooth=True) (sinc(rad / (s0 + 1e-5))): the float32 phase bit for bit, the exciter within 1e-6"""
    from ddsp_svc_amd import synth
    f0 = P.pitch_f0(regime, 3, 40, seed=17)
    st = synth.fast_source(T_(f0, dev), SR, HOP, want_combtooth=True)
    comb, pf, acc = O.fast_source_gen(f0, SR, HOP)
    assert np.array_equal(N_(st.phase_frames)[..., 0], pf) and np.array_equal(N_(st.rad_acc), acc)
    err = np.abs(N_(st.combtooth) - comb).max()
    assert err <= 1e-6, (regime, err)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("noskip", [0, 1])
@pytest.mark.parametrize("regime", ["nyquist", "jumps", "floor_ceiling"])
def test_sinusoid_bank_rows_at_nyquist(dev, regime, noskip, knobs):
    """SinusoidBankFunction's forward where harmonics sit exactly on Nyquist (masked) next to one ulp below (not), and across octave
    jumps (a harmonic masked in one frame of a hop and not the other), with and without the skip of masked blocks (with it: against
    the oracle minus what the skip leaves out): the tails' two bars.  (test_parity.py's 5e-6 does not hold here: at 12.5 Hz all 256
    harmonics are below Nyquist and the reference's float32 rounding of k * phase, which the oracle reproduces and the bank does
    not, is worth 7e-6 of the utterance.)"""
    from ddsp_svc_amd import synth
    knobs("SINS_NOSKIP", noskip)
    B, F, H = 3, 32, 256
    f0 = P.pitch_f0(regime, B, F, seed=18)
    (c,) = P.pitch_controls(B, F, [H], "unit", seed=19)
    st = synth.phase(T_(f0, dev), SR, HOP)
    out = N_(synth.SinusoidBankFunction.apply(T_(f0, dev), st, T_(c, dev), SR, HOP))
    x, _ = O.wrapped_phase(f0, SR, HOP)
    ref = O.sinusoid_bank(x, f0, c, SR, HOP)
    if not noskip:
        ref = ref - P.sins_skipped_bank(x, f0, c, SR, HOP)
    P.judge(out, ref, HOP, what=(regime, noskip))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("in_kernel_noise", [False, True])
def test_sine_source_full_range(dev, in_kernel_noise):
    """nsf_source.sine_source at dim 9 with f0 up to 4 400 Hz (harmonics 2 .. 9 above Nyquist from 2 450 Hz), unvoiced frames, the
    noise supplied or drawn in the kernel: max abs 2e-6"""
    from ddsp_svc_amd import nsf_source as S
    B, L, dim = 3, 40, 9
    f0 = np.concatenate([P.pitch_f0("glide", 1, L, seed=20), P.pitch_f0("jumps", 2, L, seed=20)[1:],
                         P.pitch_f0("floor_ceiling", 2, L)[1:]])[..., 0].copy()
    f0[0, 5:8] = 0.0
    rng = np.random.default_rng(21)
    w = rng.standard_normal(dim).astype(np.float32) * 0.3
    b = rng.standard_normal(1).astype(np.float32) * 0.1
    ri = rng.random(dim).astype(np.float32)
    ri[0] = 0
    t = lambda a: T_(a, dev)
    if in_kernel_noise:
        out = S.sine_source(t(f0), HOP, SR, t(w), t(b), t(ri), None, noise_seed=5, noise_offset=1)
        nz = N_(S.normal_noise(B, L * HOP, dim, 5, 1, dev))
    else:
        nz = rng.standard_normal((B, L * HOP, dim)).astype(np.float32)
        out = S.sine_source(t(f0), HOP, SR, t(w), t(b), t(ri), t(nz))
    ref = O.sine_source(f0, HOP, SR, w, b, ri, nz)
    assert np.abs(N_(out) - ref).max() <= 2e-6


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("tag", ["fastsrc", "sinesrc"])
def test_primitives_against_pitch_range_golden(dev, golden_dir, tag):
    """fast_source's exciter and the NSF source against the reference's own output at 12.5 .. 4 400 Hz"""
    from ddsp_svc_amd import nsf_source as S, synth
    g = _load(golden_dir, f"pitch_{tag}.npz")
    dec = int(g["dec"])
    if tag == "fastsrc":
        st = synth.fast_source(T_(g["f0_frames"], dev), SR, HOP, want_combtooth=True)
        assert np.array_equal(N_(st.phase_frames)[..., 0], g["phase_frames"])
        assert np.abs(N_(st.combtooth)[:, ::dec] - g["combtooth"]).max() <= 1e-6
    else:
        f0 = g["f0"]
        nz = np.random.default_rng(int(g["noise_seed"])).standard_normal((f0.shape[0], f0.shape[1] * HOP, 9)).astype(np.float32)
        out = S.sine_source(T_(f0, dev), HOP, SR, T_(g["weight"], dev), T_(g["bias"], dev), T_(g["rand_ini"], dev), T_(nz, dev))
        assert np.abs(N_(out)[:, ::dec] - g["out"]).max() <= 4e-6        # 2e-6 to the oracle + the oracle's 2e-6 to the reference


# ================================================================================================================================
# 6. gradients at the range a raised f0_max sees in training: 50 .. 1 600 Hz with octave jumps
# ================================================================================================================================
def _train_f0(B, F, seed):
    """50 .. 1 600 Hz: octave / two-octave jumps, and exact-Nyquist frames of k = 14 (1 575 Hz), 21, 25, 50, 63"""
    j = P.pitch_f0("jumps", 3, F, seed=seed)[..., 0]
    rows = [np.clip(j[0], 50, 1600), np.clip(j[1], 50, 1600), np.clip(j[2] * 4, 50, 1600)]
    rng = np.random.default_rng(seed)
    for k in (14, 21, 25, 50, 63):
        exact = P.nyquist_f0(k)[0]
        row = np.full(F, exact, np.float32)
        row[rng.random(F) < 0.4] = np.nextafter(exact, np.float32(0))
        row[:2] = np.float32(exact * 0.71)
        rows.append(row)
    return np.stack(rows[:B]).astype(np.float32)[:, :, None]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("rows", [(0, 3), (1, 4), (2, 5, 6, 7)])
def test_sinusoid_bank_adjoint_training_range(dev, rows):
    """SinusoidBankFunction's adjoint (its mask is the Nyquist test f0 k < sr / 2) against O.sinusoid_bank_backward: 1e-5"""
    from ddsp_svc_amd import synth
    F, H = 12, 128
    f0 = _train_f0(8, F, seed=22)[list(rows)]
    B = f0.shape[0]
    (c,) = P.pitch_controls(B, F, [H], "unit", seed=23)
    R = np.random.default_rng(24).standard_normal((B, F * HOP)).astype(np.float32)
    st = synth.phase(T_(f0, dev), SR, HOP)
    cc = T_(c, dev).requires_grad_(True)
    (synth.SinusoidBankFunction.apply(T_(f0, dev), st, cc, SR, HOP) * T_(R, dev)).sum().backward()
    xw, _ = O.wrapped_phase(f0, SR, HOP)
    want = O.sinusoid_bank_backward(R, xw, f0, c, SR, HOP)
    got = N_(cc.grad)
    for b in range(B):
        assert rms(got[b] - want[b]) <= 1e-5 * rms(want[b]), (rows, b, rms(got[b] - want[b]), rms(want[b]))


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_combsub_tail_adjoint_training_range(dev):
    """the CombSub fused tail's control gradients (one autograd node, 256 bins, hop 512) against O.combsub_dsp_backward at
    50 .. 1 600 Hz: 2e-5, test_fused_tail_training_node's bar"""
    from ddsp_svc_amd import synth
    B, F, n = 3, 9, 256
    f0 = _train_f0(8, F, seed=25)[[0, 1, 3]]
    ctrls = P.pitch_controls(B, F, [n, n, n], "unit", seed=26)
    u = np.random.default_rng(27).random((B, F * HOP)).astype(np.float32)
    R = np.random.default_rng(28).standard_normal((B, F * HOP)).astype(np.float32)
    c = [T_(x, dev).requires_grad_(True) for x in ctrls]
    st = synth.phase(T_(f0, dev), SR, HOP)
    sig, _, _ = synth.combsub_synth(T_(f0, dev), st, c[0], c[1], c[2], T_(u, dev), SR, HOP, noise_is_u01=True)
    assert "CombSubTail" in type(sig.grad_fn).__name__
    grads = torch.autograd.grad((sig * T_(R, dev)).sum(), c)
    want = O.combsub_dsp_backward(R, f0, ctrls[0], ctrls[1], ctrls[2], 2.0 * u - 1.0)
    for g_, k in zip(grads, ("group_delay", "harmonic_magnitude", "noise_magnitude")):
        e, r = rms(N_(g_) - want[k]), rms(want[k])
        assert e <= 2e-5 * r, (k, e, r)
