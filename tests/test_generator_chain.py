"""The NSF-HiFiGAN generator above the single kernel: ``nsf_generator.generator_forward`` -- the code ``patch_reference_generator``
binds -- and the dispatchers ``seam_forward`` / ``stage_forward`` / ``head_forward`` on a stand-in generator
(tests/generator_standin.py) in two topologies, on the emulator and on the GPU: "a", the stock vocoder's tail (a 256 -> 128 stage
on torch handing over to the 64-, 32- and 16-channel stages on HIP, u = 2, s = 4, 2, 1), and "b" (u = 8 and 4 in a chain, the
64-column seam tile, a 32-channel head).

The float64 oracle chain is pinned to the reference's own ``Generator`` through tests/golden/generator_chain_{a,b}.npz at 1e-5 of
the RMS.  The parity bar is the one of test_resblock.py and test_generator_tail.py: with e_torch = max|the float32 torch line on
the CPU - oracle| for the same step (for the whole chain: the stand-in's own torch forward), the HIP path must stay within
4 e_torch + 1e-7 rms(oracle).  Against the fixture, which is itself a float32 torch result e_torch away from the oracle, the bar is
one e_torch more (the triangle inequality).

Everything that must be equal "to the bit" compares two runs of the same kernels on the same values: a kernel's result depends on
neither the utterance's index, the strides its input arrived with, the stream it ran on, nor what the caches held before.
"""
import os

import numpy as np
import pytest
import torch

from tests import generator_standin as S
from tests import generator_tail_oracle as TO
from tests import resblock_oracle as BO
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import _ffi
from ddsp_svc_amd import nsf_generator as NG  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generator_chain_%s.npz")
NAMES = ("a", "b")
COUNTERS = ("hip", "reference", "seam_hip", "seam_reference", "head_hip", "head_reference")
EXPECTED = {"a": (9, 3, 3, 1, 1, 0), "b": (6, 0, 2, 0, 1, 0)}
_CASES = {}


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def _case(name):
    """the fixture, the seeded weights, the float64 chain on the fixture's inputs and the stand-in on the CPU: made once"""
    if name not in _CASES:
        g = dict(np.load(GOLDEN % name))
        w = S.weights(name)
        cpu = S.build(name)
        _CASES[name] = dict(g=g, w=w, rec=S.oracle_chain(w, g["mel"], g["source"], S.TOPOLOGIES[name]["rates"]), cpu=cpu)
    return _CASES[name]


def _counts():
    return tuple(NG.CALLS[c] for c in COUNTERS)


def _delta(before):
    return tuple(b - a for a, b in zip(before, _counts()))


def _params(names=NAMES):
    out = []
    for backend in BACKENDS:
        emu = backend == "emu"
        for name in names:
            out.append(pytest.param(backend, name, marks=[] if emu else [pytest.mark.gpu], id="%s-%s" % ("emu" if emu else "gpu", name)))
    return out


def _inputs(gen, device, mel, f0, source):
    """the three inputs on ``device``, the source stored in the stand-in's ``m_source``"""
    gen.m_source.value = torch.from_numpy(np.ascontiguousarray(source)).to(device)
    return torch.from_numpy(np.ascontiguousarray(mel)).to(device), torch.from_numpy(np.ascontiguousarray(f0)).to(device)


def _lines(gen, f0):
    """``generator_forward``'s lines after the source, as ``(boundary, function of the boundary before)``"""
    source = gen.m_source(f0, gen.upp).transpose(1, 2)
    lines = [("pre", gen.conv_pre)]
    for i in range(len(gen.ups)):
        lines.append(("seam_%d" % i, lambda x, i=i: NG.seam_forward(gen.ups[i], gen.noise_convs[i], x, source)))
        lines.append(("stage_%d" % i, lambda x, i=i: NG.stage_forward(gen.stage_blocks(i), x)))
    return lines + [("out", lambda x: NG.head_forward(gen.conv_post, x))]


def _steps(gen, mel, f0):
    """``generator_forward`` line by line, every boundary kept: ``pre``, ``seam_<i>``, ``stage_<i>``, ``out``"""
    rec, x = {}, mel
    for key, line in _lines(gen, f0):
        x = rec[key] = line(x)
    return rec


def _walk(gen, first, f0, want, what):
    """Another run of the chain against the boundaries ``want`` of an earlier run, line by line.  The lines that torch runs
    (``conv_pre`` always, the 256 -> 128 stage of "a") are not the project's to hold to the bit: torch's convolutions pick their
    algorithm by the batch size and, on the GPU, do not return the same bits from one call to the next.  They are held to 1e-5 of
    the RMS, and every line continues from the earlier run's boundary, so that each line on HIP sees identical inputs in both
    runs and must return identical bits, up to the output.  Returns the boundaries torch ran."""
    x, on_torch = first, []
    for key, line in _lines(gen, f0):
        before = _counts()
        y = line(x)
        d = _delta(before)
        assert tuple(y.shape) == tuple(want[key].shape), (what, key)
        if key == "pre" or d[1] or d[3] or d[5]:
            on_torch.append(key)
            assert (y - want[key]).abs().max() <= 1e-5 * _rms(_np64(want[key])), (what, key)
        else:
            assert torch.equal(y, want[key]), (what, key)
        x = want[key]
    return on_torch


ON_TORCH = {"a": ["pre", "seam_0", "stage_0"], "b": ["pre"]}


def _recorded_forward(monkeypatch, gen, mel, f0):
    """``generator_forward`` with every dispatcher call it makes written down: ``(boundaries, calls)``, the calls as (dispatcher,
    the modules handed over)"""
    bounds, calls = {}, []
    seam, stage, head = NG.seam_forward, NG.stage_forward, NG.head_forward

    def rec_seam(up, noise, x, source):
        bounds.setdefault("pre", x)
        i = sum(c[0] == "seam" for c in calls)
        calls.append(("seam", (up, noise)))
        y = bounds["seam_%d" % i] = seam(up, noise, x, source)
        return y

    def rec_stage(blocks, x):
        i = sum(c[0] == "stage" for c in calls)
        calls.append(("stage", tuple(blocks)))
        y = bounds["stage_%d" % i] = stage(blocks, x)
        return y

    def rec_head(post, x):
        calls.append(("head", (post,)))
        y = bounds["out"] = head(post, x)
        return y
    with monkeypatch.context() as m:
        m.setattr(NG, "seam_forward", rec_seam)
        m.setattr(NG, "stage_forward", rec_stage)
        m.setattr(NG, "head_forward", rec_head)
        out = NG.generator_forward(gen, mel, f0)
    assert out is bounds["out"]
    return bounds, calls


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _module_weights(gen):
    """``generator_standin.weights``' layout, read back from a module (after an in-place update)"""
    a = lambda t: t.detach().cpu().numpy()
    n = gen.num_kernels
    seams = [(a(u.weight), a(u.bias), a(c.weight), a(c.bias)) for u, c in zip(gen.ups, gen.noise_convs)]
    blocks = [[([(a(c1.weight), a(c1.bias), a(c2.weight), a(c2.bias)) for c1, c2 in zip(b.convs1, b.convs2)], S.DILATIONS)
               for b in gen.resblocks[i * n:(i + 1) * n]] for i in range(len(gen.ups))]
    return dict(pre=(a(gen.conv_pre.weight), a(gen.conv_pre.bias)), seams=seams, blocks=blocks,
                head=(a(gen.conv_post.weight), a(gen.conv_post.bias)))


def _check_step(what, got, ref, torch_line):
    err, e_torch, rms = float(np.abs(_np64(got) - ref).max()), float(np.abs(_np64(torch_line) - ref).max()), _rms(ref)
    bar = 4.0 * e_torch + 1e-7 * rms
    print("%s: hip %.3e torch %.3e bar %.3e ratio to torch %.2f" % (what, err, e_torch, bar, err / max(e_torch, 1e-30)))
    assert tuple(got.shape) == ref.shape and err <= bar, (what, err, e_torch, bar)
    return err / max(e_torch, 1e-30)


def _stagewise(name, gen, cpu, device, x_pre, source, only=None):
    """every seam, every stage and the head through the dispatchers, each fed the float32 rounding of the oracle's input at its
    boundary and held to the bar against the oracle's step on that same rounded input"""
    w = _module_weights(cpu)
    rates = S.TOPOLOGIES[name]["rates"]
    src64 = np.asarray(source, np.float64).reshape(source.shape[0], -1)
    src_cpu = torch.from_numpy(np.ascontiguousarray(source)).transpose(1, 2)
    src_dev = torch.from_numpy(np.ascontiguousarray(source)).to(device).transpose(1, 2)
    x64 = np.asarray(x_pre, np.float64)
    for i, u in enumerate(rates):
        s = int(np.prod(rates[i + 1:]))
        x32 = x64.astype(np.float32)
        ref = TO.seam(x32, *w["seams"][i][:2], u, src64, *w["seams"][i][2:], s)
        if only is None or i in only:
            _check_step("%s seam %d" % (name, i), NG.seam_forward(gen.ups[i], gen.noise_convs[i], torch.from_numpy(x32).to(device), src_dev),
                        ref, cpu.torch_seam(i, torch.from_numpy(x32), src_cpu))
        x32 = ref.astype(np.float32)
        ref = BO.stage(x32, w["blocks"][i])
        if only is None or i in only:
            _check_step("%s stage %d" % (name, i), NG.stage_forward(gen.stage_blocks(i), torch.from_numpy(x32).to(device)),
                        ref, cpu.torch_stage(i, torch.from_numpy(x32)))
        x64 = ref
    if only is None:
        x32 = x64.astype(np.float32)
        _check_step("%s head" % name, NG.head_forward(gen.conv_post, torch.from_numpy(x32).to(device)), TO.head(x32, *w["head"]),
                    cpu.torch_head(torch.from_numpy(x32)))


# ---- 1. the oracle chain against the reference's own generator ----------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_oracle_chain_matches_reference_fixture(name):
    c = _case(name)
    g, rec = c["g"], c["rec"]
    assert os.path.getsize(GOLDEN % name) < 200000
    topo = S.TOPOLOGIES[name]
    assert g["mel"].shape == (2, S.MELS, topo["frames"]) and g["source"].shape == (2, topo["frames"] * S.upp(name), 1)
    for i, (C, u, s) in enumerate(S.stages(name)):
        seam, stage, noise = rec["seam_%d" % i], rec["stage_%d" % i], rec["noise_%d" % i]
        assert stage.shape == (2, C, topo["frames"] * int(np.prod(topo["rates"][:i + 1])))
        # neither term of a sum hides behind the other: the noise conv in the seam, the blocks' conv terms beside the residual
        assert _rms(noise) > 0.1 * _rms(seam) and _rms(seam - noise) > 0.1 * _rms(seam), (i, _rms(noise), _rms(seam))
        assert _rms(stage - seam) > 0.1 * _rms(stage) and _rms(seam) > 0.1 * _rms(stage), (i, _rms(stage - seam), _rms(stage))
        got = g["stage_%d" % i].astype(np.float64)     # utterance 0 only (make_golden_generator_chain.py)
        assert got.shape == stage[0].shape and np.abs(got - stage[0]).max() <= 1e-5 * _rms(stage[0]), i
    assert g["out"].shape == rec["out"].shape == (2, 1, topo["frames"] * S.upp(name))
    assert np.abs(g["out"] - rec["out"]).max() <= 1e-5 * _rms(rec["out"])
    assert 0.05 < _rms(rec["out"]) < 0.9               # tanh neither linear around a bias nor saturated
    with torch.no_grad():                              # the stand-in's torch forward IS the reference's: the same float32 ops
        mel, f0 = _inputs(c["cpu"], "cpu", g["mel"], g["f0"], g["source"])
        assert torch.equal(c["cpu"](mel, f0), torch.from_numpy(g["out"]))


def test_standin_names_the_tables_stages():
    assert S.stages("a") == [(128, 2, 8), (64, 2, 4), (32, 2, 2), (16, 2, 1)] and S.stages("b") == [(64, 8, 4), (32, 4, 1)]
    assert S.upp("a") == 16 and S.upp("b") == 32


# ---- 2. every step through its dispatcher ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev,name", _params(), indirect=["dev"])
def test_stagewise_parity(dev, name):
    c = _case(name)
    gen = S.build(name, dev)
    if name == "a":                                    # T = 96, 192, 384 cross the blocks' tiles (128 - (k - 1)) and the seam's
        assert NG.tile(64, 11) < 192 and NG.tile(16, 3) < 384 and NG.seam_tile(32, 2) < 192
    else:
        assert NG.seam_tile(64, 8) == 64
    before = _counts()
    _stagewise(name, gen, c["cpu"], dev, c["rec"]["pre"], c["g"]["source"])
    assert _delta(before) == EXPECTED[name]            # and every step took the line the table names


# ---- 3. the whole chain -----------------------------------------------------------------------------------------------------------------

def _forward(name, device, gen=None):
    c = _case(name)
    gen = S.build(name, device) if gen is None else gen
    mel, f0 = _inputs(gen, device, c["g"]["mel"], c["g"]["f0"], c["g"]["source"])
    return gen, mel, f0


@pytest.mark.parametrize("dev,name", _params(), indirect=["dev"])
def test_whole_chain_parity(dev, name):
    c = _case(name)
    exact, fixture = c["rec"]["out"], c["g"]["out"].astype(np.float64)
    gen, mel, f0 = _forward(name, dev)
    before = _counts()
    got = _np64(NG.generator_forward(gen, mel, f0))
    assert _delta(before) == EXPECTED[name]
    e_torch, rms = float(np.abs(fixture - exact).max()), _rms(exact)
    err, err_fix = float(np.abs(got - exact).max()), float(np.abs(got - fixture).max())
    print("chain %s: hip %.3e torch %.3e ratio to torch %.2f; against the fixture %.3e; rms %.3f" % (
        name, err, e_torch, err / e_torch, err_fix, rms))
    assert got.shape == exact.shape
    assert err <= 4.0 * e_torch + 1e-7 * rms, (err, e_torch)
    assert err_fix <= 5.0 * e_torch + 1e-7 * rms, (err_fix, e_torch)
    assert 0.05 < _rms(got) < 0.9


# ---- 4. generator_forward is its lines -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev,name", _params(), indirect=["dev"])
def test_step_by_step_equals_generator_forward(dev, name, monkeypatch):
    """``generator_forward`` hands the modules of stage i, in order, to the three dispatchers, and the step-by-step path
    reproduces every boundary of it: to the bit where the line ran on HIP (``_walk``)"""
    gen, mel, f0 = _forward(name, dev)
    bounds, calls = _recorded_forward(monkeypatch, gen, mel, f0)
    n = len(gen.ups)
    want = []
    for i in range(n):
        want += [("seam", (gen.ups[i], gen.noise_convs[i])), ("stage", tuple(gen.resblocks[3 * i:3 * i + 3]))]
    assert [c[0] for c in calls] == [w[0] for w in want] + ["head"]
    for (_, got), (_, mods) in zip(calls, want + [("head", (gen.conv_post,))]):
        assert len(got) == len(mods) and all(a is b for a, b in zip(got, mods))
    assert list(bounds) == [k for k, _ in _lines(gen, f0)]
    assert _walk(gen, mel, f0, bounds, name) == ON_TORCH[name]
    exact = _case(name)["rec"]
    for key, t in bounds.items():                      # the boundaries are the oracle's, not only the end
        assert np.abs(_np64(t) - exact[key]).max() <= 1e-4 * _rms(exact[key]), key
    if name == "a":                                    # the HIP stages alone, behind the torch stage's real output: bit for bit
        tail, x0 = S.Tail(gen, 1), bounds["stage_0"]
        before = _counts()
        whole = NG.generator_forward(tail, x0, f0)
        assert _delta(before) == (9, 0, 3, 0, 1, 0)
        assert torch.equal(_steps(tail, x0, f0)["out"], whole) and torch.equal(whole, bounds["out"])


# ---- 5. which line every step took --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev,name", _params(), indirect=["dev"])
def test_dispatch_accounting(dev, name):
    c = _case(name)
    gen, mel, f0 = _forward(name, dev)
    assert torch.is_grad_enabled() and not any(p.requires_grad for p in gen.parameters())
    before = _counts()
    out = NG.generator_forward(gen, mel, f0)
    assert dict(zip(COUNTERS, _delta(before))) == dict(zip(COUNTERS, EXPECTED[name]))
    gen.ups[-1].weight.requires_grad_(True)            # a gradient is wanted: the whole call is the fallback's
    before = _counts()
    fell = NG.generator_forward(gen, mel, f0)
    assert _delta(before) == (0,) * 6 and fell.requires_grad
    with torch.no_grad():
        assert (fell - gen(mel, f0)).abs().max() <= 1e-5 * _rms(_np64(fell))       # torch's chain twice: its bits are torch's affair
        before = _counts()
        again = NG.generator_forward(gen, mel, f0)     # no gradient is recorded here: HIP again
        assert _delta(before) == EXPECTED[name] and (again - out).abs().max() <= 1e-5 * _rms(_np64(out))
    sentinel = object()
    assert NG.generator_forward(gen, mel, f0, fallback=lambda g, x, f: sentinel) is sentinel
    gen.ups[-1].weight.requires_grad_(False)
    i = [C for C, _, _ in S.stages(name)].index(32)    # one block of the 32-channel stage handed to the torch line
    x32 = c["rec"]["seam_%d" % i].astype(np.float32)
    ref = BO.stage(x32, c["w"]["blocks"][i])
    NG.TORCH_FASTER[(32, 7)] = None
    try:
        before = _counts()
        got = NG.stage_forward(gen.stage_blocks(i), torch.from_numpy(x32).to(dev))
        assert _delta(before) == (2, 1, 0, 0, 0, 0)
    finally:
        del NG.TORCH_FASTER[(32, 7)]
    _check_step("%s stage %d, k = 7 on torch" % (name, i), got, ref, c["cpu"].torch_stage(i, torch.from_numpy(x32)))


def test_generator_forward_falls_back_as_a_whole():
    """host tensors, another dtype, a first block without ``convs1`` / ``convs2``, a missing attribute: the fallback, untouched"""
    gen, mel, f0 = _forward("b", "cpu")
    calls = []
    fb = lambda g, x, f: calls.append((g, x, f)) or "fallback"
    before = _counts()
    assert NG.generator_forward(gen, mel, f0, fallback=fb) == "fallback" and calls[-1][1] is mel      # no GPU tensor
    with torch.no_grad():
        assert torch.equal(NG.generator_forward(gen, mel, f0), gen(mel, f0))                           # fallback None: its own forward
    assert _delta(before) == (0,) * 6


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_generator_forward_duck_types(dev):
    gen, mel, f0 = _forward("b", dev)
    fb = lambda g, x, f: "fallback"
    before = _counts()
    assert NG.generator_forward(gen, mel.double(), f0, fallback=fb) == "fallback"
    first = gen.resblocks[0]
    plain = torch.nn.Module()
    plain.convs = first.convs1                         # ResBlock2's shape: one list of convs
    gen.resblocks[0] = plain
    assert NG.generator_forward(gen, mel, f0, fallback=fb) == "fallback"
    gen.resblocks[0] = first
    upp = gen.upp
    del gen.upp
    assert NG.generator_forward(gen, mel, f0, fallback=fb) == "fallback"
    gen.upp = upp
    assert _delta(before) == (0,) * 6
    assert NG.generator_forward(gen, mel, f0, fallback=fb).shape == (2, 1, 640) and _delta(before) == EXPECTED["b"]


# ---- 6. inputs as torch hands them over ---------------------------------------------------------------------------------------------------

def _layouts(x):
    """``x`` again with the same values: every second row of a 2 B tensor, and channels-last memory"""
    twice = torch.full((2 * x.shape[0],) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype, device=x.device)
    twice[::2] = x
    last = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not twice[::2].is_contiguous() and (x.shape[2] == 1 or not last.is_contiguous())
    return {"batch-strided": twice[::2], "channels-last": last}


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_inputs_as_torch_hands_them_over(dev):
    gen, mel, f0 = _forward("a", dev)
    stored = gen.m_source(f0, gen.upp)                  # [B, L upp, 1]
    source = stored.transpose(1, 2)                     # the view generator_forward makes
    assert source.shape == (2, 1, 384) and source.data_ptr() == stored.data_ptr()
    with torch.no_grad():
        x = gen.torch_stage(0, gen.torch_seam(0, gen.conv_pre(mel), source))       # what the torch 256 -> 128 stage really returns
    assert x.shape == (2, 128, 48)
    before = _counts()
    want = NG.seam_forward(gen.ups[1], gen.noise_convs[1], x.contiguous().clone(), source.contiguous().clone())
    assert torch.equal(NG.seam_forward(gen.ups[1], gen.noise_convs[1], x, source), want)
    src2 = torch.full((4, 384, 1), float("nan"), device=dev)
    src2[::2] = stored
    for how, v in _layouts(x).items():
        assert torch.equal(NG.seam_forward(gen.ups[1], gen.noise_convs[1], v, source), want), how
        assert torch.equal(NG.seam_forward(gen.ups[1], gen.noise_convs[1], v, src2[::2].transpose(1, 2)), want), how
    up, nz = gen.ups[1], gen.noise_convs[1]
    for how, v in _layouts(x).items():                  # the functional forms, into a NaN-prefilled ``out``
        out = torch.full_like(want, float("nan"))
        assert NG.upsample_stage(v, up.weight, up.bias, 2, source, nz.weight, nz.bias, 4, out=out) is out and torch.equal(out, want), how
    staged = NG.stage_forward(gen.stage_blocks(1), want)
    spec = [NG._block_spec(b) for b in gen.stage_blocks(1)]
    for how, v in _layouts(want).items():
        assert torch.equal(NG.stage_forward(gen.stage_blocks(1), v), staged), how
        out = torch.full_like(want, float("nan"))
        assert torch.equal(NG.resblock1(v, spec[2][0], spec[2][1], out=out), NG.resblock1(want, spec[2][0], spec[2][1])), how
    assert not torch.isnan(staged).any()
    x3 = NG.stage_forward(gen.stage_blocks(3), NG.seam_forward(gen.ups[3], gen.noise_convs[3], NG.stage_forward(
        gen.stage_blocks(2), NG.seam_forward(gen.ups[2], gen.noise_convs[2], staged, source)), source))
    head = NG.head_forward(gen.conv_post, x3)
    for how, v in _layouts(x3).items():
        assert torch.equal(NG.head_forward(gen.conv_post, v), head), how
        out = torch.full_like(head, float("nan"))
        assert torch.equal(NG.output_head(v, gen.conv_post.weight, gen.conv_post.bias, out=out), head), how
    d = _delta(before)
    assert d[1] == 0 and d[3] == 0 and d[5] == 0        # every one of these calls ran on HIP
    assert np.abs(_np64(head) - _case("a")["rec"]["out"]).max() <= 1e-4


# ---- 7. rows are independent ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev,name", _params(), indirect=["dev"])
def test_rows_are_independent(dev, name):
    """Row b of a B = 3 run against the B = 1 run of that row, at every boundary (``_walk``: torch's convolution picks its
    algorithm by the batch size, on the CPU already)"""
    frames = S.TOPOLOGIES[name]["frames"]
    mel, f0, source = S.seeded_inputs(name, 3, frames, seed=7)
    assert np.abs(mel[0] - mel[1]).max() > 0.5 and np.abs(source[1] - source[2]).max() > 0.5          # different utterances
    gen = S.build(name, dev)
    m, f = _inputs(gen, dev, mel, f0, source)
    together = {k: v.clone() for k, v in _steps(gen, m, f).items()}
    assert together["out"].shape == (3, 1, frames * S.upp(name))
    for b in range(3):
        m, f = _inputs(gen, dev, mel[b:b + 1], f0[b:b + 1], source[b:b + 1])
        assert _walk(gen, m, f, {k: v[b:b + 1] for k, v in together.items()}, "row %d" % b) == ON_TORCH[name]


# ---- 8. lengths vary within one process ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_lengths_vary_with_the_caches_kept(dev):
    name, lengths = "a", (24, 7, 40, 1, 24)
    gen = S.build(name, dev)
    cases = [S.seeded_inputs(name, 2, L, seed=L) for L in lengths]
    NG.release_workspace()
    NG.clear_packed()
    kept = []
    for mel, f0, source in cases[:4]:
        m, f = _inputs(gen, dev, mel, f0, source)
        kept.append({k: v.clone() for k, v in _steps(gen, m, f).items()})
    m, f = _inputs(gen, dev, *cases[4])                # 24 again, behind 1 and 40: the caches as the other lengths left them
    assert _walk(gen, m, f, kept[0], "24 again") == ON_TORCH[name]
    assert len(NG._WS) == 1
    grown = next(iter(NG._WS.values())).numel()
    assert grown * 4 == 2 * 2 * 16 * 40 * 16 * 4        # two [2, 16, 640] activations: the largest shape seen, never shrunk
    for L, (mel, f0, source), got in zip(lengths, cases, kept):
        NG.release_workspace()
        NG.clear_packed()
        m, f = _inputs(gen, dev, mel, f0, source)
        assert got["out"].shape == (2, 1, 16 * L) and _walk(gen, m, f, got, "L = %d, cleared caches" % L) == ON_TORCH[name]
    cpu = S.build(name)
    with torch.no_grad():                              # one residual-block weight and one seam weight written in place
        for g in (gen, cpu):
            g.stage_blocks(2)[1].convs2[1].weight.mul_(-1.5)
            g.ups[2].weight.mul_(-1.5)
    mel, f0, source = cases[0]
    m, f = _inputs(gen, dev, mel, f0, source)
    after = NG.generator_forward(gen, m, f)
    assert (after - kept[0]["out"]).abs().max() > 1e-3
    pre = BO.conv1d(mel, *_case(name)["w"]["pre"], 1, 3)
    _stagewise(name, gen, cpu, dev, pre, source, only=(2,))


# ---- 11. one hand-over buffer per stream -------------------------------------------------------------------------------------------------------

def test_workspace_is_keyed_by_device_and_stream(monkeypatch):
    """the cache's bookkeeping, without a device: one buffer per (device, stream), grown and never shrunk, all dropped by
    ``release_workspace``, at most ``_WS_MAX`` kept"""
    stream = [1]
    monkeypatch.setattr(_ffi, "stream_of", lambda t: stream[0])
    NG.release_workspace()
    x = torch.zeros(1)
    a = NG._workspace(64, x)
    assert a.numel() == 16 and NG._workspace(32, x) is a and NG._workspace(64, x) is a
    stream[0] = 2
    b = NG._workspace(64, x)
    assert b is not a and b.data_ptr() != a.data_ptr() and len(NG._WS) == 2
    big = NG._workspace(4096, x)
    assert big.numel() == 1024 and big is not b and NG._workspace(64, x) is big
    stream[0] = 1
    assert NG._workspace(64, x) is a
    for s in range(3, 3 + NG._WS_MAX):
        stream[0] = s
        NG._workspace(16, x)
    assert len(NG._WS) == NG._WS_MAX and ("cpu", 2) not in NG._WS
    NG.release_workspace()
    assert len(NG._WS) == 0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stage64(device, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 64, T, generator=g).to(device)


@pytest.mark.gpu
def test_gpu_two_streams_get_two_buffers():
    """After one call on each of two streams ``_WS`` holds two buffers at different addresses: the deterministic check of the
    one-buffer-per-stream rule, and the one that fails where a single buffer per device is shared (a concurrent run cannot be
    relied on to show the shared buffer: the launches are short and mostly do not overlap).  Then both streams run the
    64-channel stage of topology "a" eight times side by side and must reproduce their serial results to the bit."""
    device = _need_gpu()
    gen = S.build("a", device)
    blocks = gen.stage_blocks(1)
    x1, x2 = _stage64(device, 4096, 1), _stage64(device, 4096 + 77, 2)
    serial = [NG.stage_forward(blocks, x1).clone(), NG.stage_forward(blocks, x2).clone()]
    torch.cuda.synchronize()
    NG.release_workspace()
    s1, s2 = torch.cuda.Stream(device), torch.cuda.Stream(device)
    with torch.cuda.stream(s1):
        NG.stage_forward(blocks, x1)
    with torch.cuda.stream(s2):
        NG.stage_forward(blocks, x2)
    torch.cuda.synchronize()
    assert sorted(NG._WS) == sorted((str(device), s.cuda_stream) for s in (s1, s2))
    assert len({t.data_ptr() for t in NG._WS.values()}) == 2
    y1, y2 = [], []
    before = _counts()
    for _ in range(8):
        with torch.cuda.stream(s1):
            y1.append(NG.stage_forward(blocks, x1))
        with torch.cuda.stream(s2):
            y2.append(NG.stage_forward(blocks, x2))
    s1.synchronize()
    s2.synchronize()
    assert _delta(before) == (48, 0, 0, 0, 0, 0) and len(NG._WS) == 2
    assert all(torch.equal(y, serial[0]) for y in y1) and all(torch.equal(y, serial[1]) for y in y2)


# ---- 9. a stream of the caller's ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_non_default_stream():
    """The inputs come from torch ops enqueued on a side stream right before the chain, nothing is synchronised in between and
    only that stream is waited on: every launch of the chain is ordered on the caller's stream.  The chain is the three HIP
    stages and the head of "a" behind the torch stage's real output (``Tail``): torch's own lines do not return the same bits
    twice on the GPU, the project's do."""
    device = _need_gpu()
    gen, mel, f0 = _forward("a", device)
    source = gen.m_source.value
    tail, x0 = S.Tail(gen, 1), _steps(gen, mel, f0)["stage_0"]
    want = NG.generator_forward(tail, x0, f0).clone()
    big = torch.randn(2048, 2048, device=device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    before = _counts()
    with torch.cuda.stream(s):
        zero = (big @ big)[:1, :1].sum() * 0.0          # some work in front of the inputs on the side stream
        gen.m_source.value = source + zero
        got = NG.generator_forward(tail, x0 + zero, f0)
        whole = NG.generator_forward(gen, mel + zero, f0)                          # and the whole chain, torch stage included
    s.synchronize()
    assert _delta(before) == tuple(a + b for a, b in zip((9, 0, 3, 0, 1, 0), EXPECTED["a"])) and (str(device), s.cuda_stream) in NG._WS
    assert torch.equal(got, want)
    assert (whole - want).abs().max() <= 1e-5 * _rms(_np64(want))


# ---- 10. the whole chain in a graph ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_graph_replay_of_the_whole_chain():
    """Topology "b" captured after a warm-up that packs the weight tables.  A capture neither reads nor grows the hand-over
    cache -- the graph owns its buffer -- so the cache may be dropped between capture and replay."""
    device = _need_gpu()
    gen, mel, f0 = _forward("b", device)
    mel2 = torch.from_numpy(S.seeded_inputs("b", 2, 20, seed=3)[0]).to(device)
    eager, eager2 = NG.generator_forward(gen, mel, f0).clone(), NG.generator_forward(gen, mel2, f0).clone()
    assert (eager - eager2).abs().max() > 1e-2
    static = mel.clone()
    torch.cuda.synchronize()
    keys = sorted(NG._WS)
    graph = torch.cuda.CUDAGraph()
    before = _counts()
    with torch.cuda.graph(graph):
        out = NG.generator_forward(gen, static, f0)
    assert _delta(before) == EXPECTED["b"] and sorted(NG._WS) == keys
    NG.release_workspace()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(mel2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2)
