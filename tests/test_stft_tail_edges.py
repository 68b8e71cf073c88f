"""The short-time spectral tail (csrc/stft.hip: the forward kernel in its compiled forms and the inline-exciter form, the backward
kernel in its forms) at the edges its first tests leave out.  Those judge by one RMS over a whole call, with B <= 3, a (symmetric)
Hann window, controls of sigma <= 1.5 and the default compiled variant only.  Here, on both backends of tests/backends.py:

  large controls      phases of sigma 10 / 40 / 300 (raw outputs of a Linear layer, nothing bounds them) and magnitudes of sigma 3 / 6.
                      The reference's angle is the float32 product fl32(pi32 * phase); a kernel that reduces the exact pi * phase
                      leaves it by |phase| pi 2^-25 radians per bin (4.7e-6 relative RMS at sigma 40, 3.5e-5 at 300: cis_pi,
                      ddsp_common.h)
  localised error     every 512-sample block of the output, every control row of every gradient stream, and the DC and Nyquist
                      columns, each held to the bar on its own -- at odd and even frame counts, the shortest reflect case, zero
                      padding and the flush of the last pair; row F - 1, which the repeated last frame accumulates into, included
  asymmetric window   the same cases under a window with no symmetry, and the general entry (win 1024, reflect, normalised)
  noise_is_u01        through stft_filter and stft_filter_backward themselves
  batch independence  rows 0, 15, 16 and B - 1 of B = 17 / 257 are the B = 1 call's bits (the run rotation by b, b >> 4, b >> 8)
  backward run split  STFT_RUN 1 / 2 / 3 / 1000: the same bits in all four gradient streams
  backward operands   split views, a strided cotangent, noise_phase = None at win 2048
  compiled variants   STFT_WPS 2 / 3 / 4: every one within the bar and equal to the default one bit for bit
  inline exciter      combsubsuperfast_synth at F = 2, 3, 4 (zero padding, the shortest reflect case and its neighbour)
  C ABI refusals      the raw entries return their documented codes and leave the outputs alone (emulator only)

Bars (float32 path against the float64 oracle, relative RMS): 2e-6 forward, 5e-6 backward -- the project's own
(test_parity_fast.py, test_backward_fast.py).  Every figure is printed before it is asserted (``STAT name backend value bar``)."""
import copy

import numpy as np
import pytest
import torch

from oracle import ddsp_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.stft_oracle import HOP, _filter_case, _oracle_filter, asym_window, hann

SR = 44100
FWD_BAR, BWD_BAR = 2e-6, 5e-6
KEYS = ("harmonic_magnitude", "harmonic_phase", "noise_magnitude", "noise_phase")
EINVAL, ESHAPE = -1, -3                                      # include/ddsp_hip.h

GEOMS = {
    "super": dict(win=2048, reflect=True, normalize=True, nphase=True),         # CombSubSuperFast (vocoder.py:661-708)
    "fast": dict(win=1024, reflect=False, normalize=False, nphase=False),       # CombSubFast (vocoder.py:758-784)
    "general": dict(win=1024, reflect=True, normalize=True, nphase=True),       # the generic entry takes every combination
}
both = pytest.mark.parametrize("dev", BACKENDS, indirect=True)


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def T_(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def stat(name, device, value, bar):
    print("STAT %s %s %.3e %.1e" % (name, "emu" if device.type == "cpu" else "gpu", value, bar))
    return value


class Case:
    """seeded inputs of one call and, made once and then read-only, their float64 references"""

    def __init__(self, geom, B, F, seed, sigma_mag=1.0, sigma_phase=1.5, window="hann", u01=False, reflect=None, nphase=None):
        g = GEOMS[geom]
        self.win, self.normalize = g["win"], g["normalize"]
        self.reflect = g["reflect"] if reflect is None else reflect
        self.B, self.F = B, F
        self.exc, nz, self.hm, self.hp, self.nm, self.nph = _filter_case(
            B, F, self.win, seed, g["nphase"] if nphase is None else nphase, sigma_mag, sigma_phase)
        rng = np.random.default_rng(seed + 77777)
        self.cot = rng.standard_normal((B, F * HOP)).astype(np.float32)
        self.u01 = u01
        if u01:                                              # multiples of 2^-24 as torch.rand gives: 2u - 1 is exact in float32
            u = (rng.integers(0, 1 << 24, (B, F * HOP)) * 2.0 ** -24).astype(np.float32)
            self.nz_in, self.nz = u, 2.0 * u.astype(np.float64) - 1.0
        else:
            self.nz_in = self.nz = nz
        if window == "asym":
            self.w = asym_window(self.win)
        else:
            self.w = hann(self.win) if self.normalize else np.sqrt(hann(self.win)).astype(np.float32)
        self._fwd = self._bwd = None

    def fwd_ref(self):
        if self._fwd is None:
            self._fwd = _oracle_filter(self.exc, self.nz, self.hm, self.hp, self.nm, self.nph, self.win, self.w, self.reflect,
                                       self.normalize)
            self._fwd.flags.writeable = False
        return self._fwd

    def bwd_ref(self):
        if self._bwd is None:
            self._bwd = O.stft_filter_backward(self.cot, self.exc, self.nz, self.hm, self.hp, self.nm, self.nph, self.w, HOP,
                                               "reflect" if self.reflect else "constant", self.normalize)
            for a in self._bwd:
                if a is not None:
                    a.flags.writeable = False
        return self._bwd

    def row(self, b):
        """utterance b alone, as a B = 1 call"""
        one = copy.copy(self)
        for k in ("exc", "nz", "nz_in", "hm", "hp", "nm", "nph", "cot"):
            v = getattr(self, k)
            setattr(one, k, None if v is None else np.ascontiguousarray(v[b:b + 1]))
        one.B, one._fwd, one._bwd = 1, None, None
        return one


_CASES = {}


def case(*args, **kw):
    key = (args, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = Case(*args, **kw)
    return _CASES[key]


def run_fwd(c, device):
    from ddsp_svc_amd import synth
    out = synth.stft_filter(T_(c.exc, device), T_(c.nz_in, device), T_(c.hm, device), T_(c.hp, device), T_(c.nm, device),
                            None if c.nph is None else T_(c.nph, device), T_(c.w, device), HOP, pad_reflect=c.reflect,
                            normalize=c.normalize, noise_is_u01=c.u01)
    return out.cpu().numpy()


def run_bwd(c, device, controls=None, cot=None):
    from ddsp_svc_amd import synth
    hm, hp, nm, nph = controls if controls is not None else (
        T_(c.hm, device), T_(c.hp, device), T_(c.nm, device), None if c.nph is None else T_(c.nph, device))
    got = synth.stft_filter_backward(T_(c.cot, device) if cot is None else cot, T_(c.exc, device), T_(c.nz_in, device), hm, hp,
                                     nm, nph, T_(c.w, device), HOP, pad_reflect=c.reflect, normalize=c.normalize,
                                     noise_is_u01=c.u01)
    return tuple(None if a is None else a.cpu().numpy() for a in got)


def check_fwd(c, out, device, local=False):
    ref = c.fwd_ref()
    assert out.shape == ref.shape
    scale = rms(ref)
    whole = stat("fwd_rel_rms", device, rms(out - ref) / scale, FWD_BAR)
    block = 0.0
    if local:                                                # every 512-sample block against the oracle's RMS over the call
        err = (out - ref).reshape(c.B, c.F, HOP)
        block = stat("fwd_block", device, float(np.sqrt(np.mean(err * err, axis=-1)).max()) / scale, FWD_BAR)
    assert whole <= FWD_BAR and block <= FWD_BAR, (whole, block)


def check_bwd(c, got, device, local=False):
    ref = c.bwd_ref()
    worst = {}
    for a, b, k in zip(got, ref, KEYS):
        if b is None:
            assert a is None, k
            continue
        assert a.shape == b.shape == (c.B, c.F, c.win // 2 + 1), k
        err = a - b
        figs = {"bwd_rel_rms": rms(err) / rms(b)}
        if local:
            # every control row (row F - 1 collects the repeated last frame) against the stream's RMS; the DC and the Nyquist
            # column, whose imaginary cotangent is dropped, each against its own column's RMS
            figs["bwd_row"] = float(np.sqrt(np.mean(err * err, axis=-1)).max()) / rms(b)
            figs["bwd_dc"] = rms(err[..., 0]) / rms(b[..., 0])
            figs["bwd_nyquist"] = rms(err[..., -1]) / rms(b[..., -1])
        for name, v in figs.items():
            worst[name] = max(worst.get(name, 0.0), v)
            if v > BWD_BAR:
                print("over the bar: %s of %s = %.3e" % (name, k, v))
    for name, v in worst.items():
        stat(name, device, v, BWD_BAR)
    assert all(v <= BWD_BAR for v in worst.values()), worst


# ---------------------------------------------------------------- large controls
LARGE = [("phase10", 1.0, 10.0), ("phase40", 1.0, 40.0), ("phase300", 1.0, 300.0), ("mag3", 3.0, 1.5), ("mag6", 6.0, 1.5)]
LARGE_SHAPES = [("super", 2, 11), ("fast", 2, 10)]


@both
@pytest.mark.parametrize("geom,B,F", LARGE_SHAPES)
@pytest.mark.parametrize("name,sigma_mag,sigma_phase", LARGE)
def test_large_controls_forward(dev, geom, B, F, name, sigma_mag, sigma_phase):
    """Measured before cis_pi rounded pi * phase as the reference does (win 2048, emulator): 1.2e-6 at sigma 10, 4.7e-6 at 40,
    3.5e-5 at 300 against the bar of 2e-6 -- the sigma 40 and 300 cases failed."""
    c = case(geom, B, F, 31, sigma_mag=sigma_mag, sigma_phase=sigma_phase)
    check_fwd(c, run_fwd(c, dev), dev)


@both
@pytest.mark.parametrize("geom,B,F", LARGE_SHAPES)
@pytest.mark.parametrize("name,sigma_mag,sigma_phase", LARGE)
def test_large_controls_backward(dev, geom, B, F, name, sigma_mag, sigma_phase):
    """the backward kernel evaluates the same filters through the same cis_pi"""
    c = case(geom, B, F, 31, sigma_mag=sigma_mag, sigma_phase=sigma_phase)
    check_bwd(c, run_bwd(c, dev), dev)


# ---------------------------------------------------------------- localised error, symmetric and asymmetric window
LOCAL = [
    ("super", 11, True),       # odd frame count: the last pair has one live frame
    ("super", 12, False),      # even; zero padding under the istft envelope
    ("super", 3, True),        # shortest reflect case: every frame touches a boundary
    ("super", 1, False),       # T <= win/2: one pair, flushed at once
    ("fast", 10, None),
    ("fast", 9, None),
    ("fast", 2, None),
    ("general", 9, None),      # win 1024 with reflect padding and the envelope: only the generic entry reaches it
]


@both
@pytest.mark.parametrize("window", ["hann", "asym"])
@pytest.mark.parametrize("geom,F,reflect", LOCAL)
def test_forward_error_is_local(dev, geom, F, reflect, window):
    c = case(geom, 2, F, 40 + F, window=window, reflect=reflect)
    check_fwd(c, run_fwd(c, dev), dev, local=True)


@both
@pytest.mark.parametrize("window", ["hann", "asym"])
@pytest.mark.parametrize("geom,F,reflect", LOCAL)
def test_backward_error_is_local(dev, geom, F, reflect, window):
    c = case(geom, 2, F, 40 + F, window=window, reflect=reflect)
    check_bwd(c, run_bwd(c, dev), dev, local=True)


# ---------------------------------------------------------------- noise_is_u01 through the filter's own entries
@both
@pytest.mark.parametrize("geom", ["super", "fast"])
def test_noise_u01(dev, geom):
    """the raw U[0, 1) draw, 2u - 1 applied on load (vocoder.py:771): the oracle is handed 2u - 1, exact, in float64"""
    c = case(geom, 2, 5, 53, u01=True)
    assert np.all(c.nz_in >= 0) and np.all(c.nz_in < 1) and abs(float(np.mean(c.nz))) < 0.01
    check_fwd(c, run_fwd(c, dev), dev, local=True)
    check_bwd(c, run_bwd(c, dev), dev, local=True)


# ---------------------------------------------------------------- rows do not depend on the batch
@both
@pytest.mark.parametrize("geom,B", [("super", 17), ("fast", 17), ("super", 257)])
def test_rows_do_not_depend_on_the_batch(dev, geom, B, knobs):
    """STFT_RUN = 1: F = 5 makes three pairs, three runs per utterance, and the forward kernel rotates the run number by
    (b + (b >> 4) + (b >> 8)) % runs -- utterance b's samples and gradients must still be those of its B = 1 call"""
    knobs("STFT_RUN", 1)
    c = case(geom, B, 5, 61)
    fwd, bwd = run_fwd(c, dev), run_bwd(c, dev)
    for b in (0, 15, 16, B - 1):
        one = c.row(b)
        assert same_bits(run_fwd(one, dev)[0], fwd[b]), ("forward", b)
        for a, whole, k in zip(run_bwd(one, dev), bwd, KEYS):
            if whole is None:
                assert a is None
                continue
            assert same_bits(a[0], whole[b]), (k, b)


# ---------------------------------------------------------------- backward run splits
@both
@pytest.mark.parametrize("geom", ["super", "fast"])
@pytest.mark.parametrize("F", [8, 9])
def test_backward_run_split_same_bits(dev, geom, F, knobs):
    """pairs are independent and frame F rides with the last pair, whichever run holds it"""
    c = case(geom, 2, F, 70 + F)
    outs = []
    for run in (1, 2, 3, 1000):
        knobs("STFT_RUN", run)
        outs.append(run_bwd(c, dev))
    for o in outs[1:]:
        for a, b, k in zip(o, outs[0], KEYS):
            assert (a is None and b is None) or same_bits(a, b), k
    assert float(np.abs(outs[0][0]).sum()) > 0


# ---------------------------------------------------------------- backward operands
@both
def test_backward_operands(dev):
    c = case("super", 2, 6, 81)
    want = run_bwd(c, dev)
    # Unit2Control's output split into views: row stride 4 n
    packed = T_(np.concatenate([c.hm, c.hp, c.nm, c.nph], axis=-1), dev)
    views = torch.split(packed, [c.win // 2 + 1] * 4, dim=-1)
    assert views[1].stride(1) == 4 * (c.win // 2 + 1)
    for a, b, k in zip(run_bwd(c, dev, controls=views), want, KEYS):
        assert same_bits(a, b), ("views", k)
    # a cotangent that is every second column of a wider tensor
    wide = torch.zeros(c.B, 2 * c.F * HOP, device=dev)
    wide[:, ::2] = T_(c.cot, dev)
    wide[:, 1::2] = 1e9
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    for a, b, k in zip(run_bwd(c, dev, cot=strided), want, KEYS):
        assert same_bits(a, b), ("strided cotangent", k)
    # no noise phase at win 2048: nothing in the fourth place, the other three as the oracle has them
    c0 = case("super", 2, 6, 81, nphase=False)
    got = run_bwd(c0, dev)
    assert len(got) == 4 and got[3] is None
    check_bwd(c0, got, dev)


# ---------------------------------------------------------------- compiled variants
@both
@pytest.mark.parametrize("what,geom,wps", [("fwd", "super", 2), ("fwd", "super", 3), ("fwd", "super", 4), ("fwd", "fast", 2),
                                           ("fwd", "fast", 3), ("bwd", "super", 2), ("bwd", "super", 3)])
def test_compiled_variants(dev, what, geom, wps, knobs):
    """STFT_WPS picks the occupancy build of the kernel: one source, another register budget.  STFT_RUN is pinned, since the
    default split moves with the variant's workgroups per CU.  Every variant meets the oracle's bar and gives the default
    variant's bits (spills move values, they do not round them)."""
    knobs("STFT_RUN", 2)
    c = case(geom, 2, 11 if geom == "super" else 10, 91)
    run = run_fwd if what == "fwd" else run_bwd
    default = run(c, dev)
    knobs("STFT_WPS", wps)
    got = run(c, dev)
    if what == "fwd":
        check_fwd(c, got, dev, local=True)
        assert same_bits(got, default)
    else:
        check_bwd(c, got, dev, local=True)
        for a, b, k in zip(got, default, KEYS):
            assert same_bits(a, b), k


# ---------------------------------------------------------------- inline-exciter form
@both
@pytest.mark.parametrize("B,F", [(1, 2), (1, 3), (1, 4)])
def test_inline_exciter_short(dev, B, F, knobs):
    """combsubsuperfast_synth at streaming shapes makes the exciter inside the filter's load path (k_stft_filter<4, 2, true>):
    F = 2 is T <= win/2 (zero padding), F = 3 the shortest reflect case, F = 4 its neighbour.  The two-launch layout's bits
    (SMALL_PATH = 1) and the oracle's numbers."""
    from ddsp_svc_amd import synth
    f0 = O.synth_f0(B, F, SR, HOP, seed=200 + F)
    hm, hp, nm, nph = O.synth_controls(B, F, [1025] * 4, seed=F + 11)
    gz = O.synth_gauss(B, F * HOP, seed=F + 12)
    w = hann(2048)
    args = [T_(a, dev) for a in (f0, hm, hp, nm, nph, gz, w)]

    def step():
        fs = synth.fast_source(args[0], SR, HOP)
        return synth.combsubsuperfast_synth(args[0], fs, *args[1:], SR, HOP)
    a = step()
    knobs("SMALL_PATH", 1)
    b = step()
    assert torch.equal(a, b) and same_bits(a.cpu().numpy(), b.cpu().numpy())
    ref = O.combsubsuperfast_dsp(f0, hm, hp, nm, nph, gz, SR, HOP, 2048, w)["signal"]
    e = stat("inline_exciter_rel_rms", dev, rms(a.cpu().numpy() - ref) / rms(ref), FWD_BAR)
    assert e <= FWD_BAR


# ---------------------------------------------------------------- C ABI refusals
SENTINEL = -12345.5


class _Raw:
    """arguments of the raw entries ddsp_hip_stft_filter / ddsp_hip_stft_filter_backward (include/ddsp_hip.h) by name, over
    buffers large enough for every accepted value of the sizes; the outputs are filled with a sentinel"""

    def __init__(self, B=1, F=4, win=2048):
        n, T = win // 2 + 1, F * HOP
        z = lambda *s: torch.zeros(*s, dtype=torch.float32)
        self.keep = dict(exciter=z(max(B, 1), T), noise=z(max(B, 1), T), c_hmag=z(max(B, 1), F, n), c_hphase=z(max(B, 1), F, n),
                         c_nmag=z(max(B, 1), F, n), c_nphase=z(max(B, 1), F, n), window=torch.ones(win), grad_signal=z(max(B, 1), T))
        self.outs = dict(signal=z(max(B, 1), T), d_hmag=z(max(B, 1), F, n), d_hphase=z(max(B, 1), F, n),
                         d_nmag=z(max(B, 1), F, n), d_nphase=z(max(B, 1), F, n))
        for t in self.outs.values():
            t.fill_(SENTINEL)
        self.a = dict({k: t.data_ptr() for k, t in {**self.keep, **self.outs}.items()}, ld_hmag=n, ld_hphase=n, ld_nmag=n,
                      ld_nphase=n, win=win, pad_reflect=1, normalize=1, B=B, F=F, hop=HOP)

    def call(self, lib, entry, **over):
        a = dict(self.a, **over)
        head = (a["exciter"], a["noise"], 0, a["c_hmag"], a["ld_hmag"], a["c_hphase"], a["ld_hphase"], a["c_nmag"], a["ld_nmag"],
                a["c_nphase"], a["ld_nphase"], 1.0 / 128.0, a["window"], a["win"], a["pad_reflect"], a["normalize"])
        if entry == "forward":
            return lib.ddsp_hip_stft_filter(*head, a["B"], a["F"], a["hop"], a["signal"], None)
        return lib.ddsp_hip_stft_filter_backward(*head, a["grad_signal"], a["B"], a["F"], a["hop"], a["d_hmag"], a["d_hphase"],
                                                 a["d_nmag"], a["d_nphase"], None)

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t in self.outs.values())


REFUSALS = [(dict(ld_hmag=1024), EINVAL), (dict(ld_hphase=1024), EINVAL), (dict(ld_nmag=1024), EINVAL),
            (dict(ld_nphase=1024), EINVAL),                                    # a row stride below win/2 + 1, per stream
            (dict(win=2047), EINVAL),                                          # odd window
            (dict(exciter=None), EINVAL), (dict(noise=None), EINVAL), (dict(c_hmag=None), EINVAL), (dict(c_hphase=None), EINVAL),
            (dict(c_nmag=None), EINVAL), (dict(window=None), EINVAL),          # each required input
            (dict(F=2), EINVAL),                                               # reflect padding needs T > win/2
            (dict(win=512, pad_reflect=0), ESHAPE),                            # no kernel for win 512
            (dict(hop=256, pad_reflect=0), ESHAPE)]                            # ... nor for hop 256
REFUSALS_FWD = [(dict(signal=None), EINVAL)]
REFUSALS_BWD = [(dict(grad_signal=None), EINVAL), (dict(d_hmag=None), EINVAL), (dict(d_hphase=None), EINVAL),
                (dict(d_nmag=None), EINVAL),
                (dict(d_nphase=None), EINVAL), (dict(c_nphase=None), EINVAL)]  # c_nphase and d_nphase: both or neither


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_c_abi_refusals(dev, entry):
    """a refused call returns its documented code before anything is launched: the outputs keep their sentinel"""
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    raw = _Raw()
    for over, code in REFUSALS + (REFUSALS_FWD if entry == "forward" else REFUSALS_BWD):
        assert raw.call(lib, entry, **over) == code, (entry, over)
        assert raw.untouched(), (entry, over)
    # the forward entry takes no noise phase as the zero-phase filter; then its row stride is not looked at
    if entry == "forward":
        assert raw.call(lib, entry, c_nphase=None, ld_nphase=0) == 0
        assert not raw.untouched()
    else:
        assert raw.call(lib, entry) == 0 and not raw.untouched()
    # an empty batch is no error and writes nothing, whatever the pointers
    raw = _Raw(B=0)
    assert raw.call(lib, entry) == 0 and raw.untouched()
    assert raw.call(lib, entry, exciter=None, signal=None, d_hmag=None) == 0 and raw.untouched()
