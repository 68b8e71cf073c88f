"""The five model-layer hooks (``conformer``, ``attention``, ``wavenet``, ``naive_v2``, ``nsf_generator``) in the torch MODES that
real callers use: ``torch.inference_mode()`` around the call, inference tensors as inputs, inference tensors as weights (a model
built or loaded inside the mode) and ``torch.autocast``.  What is held here is the routing and the contract, not the arithmetic
(the kernels have their float64 oracles elsewhere): which path a call takes (the hooks' ``CALLS``), what the caches do
(``PACKS``, ``_modules._PACKED`` / ``_STACKED``), and that the result is, bit for bit, the one the other path to the same
numbers gives.

  inside the mode, ordinary weights   the kernels, the tables cached and found again outside the mode
  inference-tensor inputs             the kernels, the same bits as with ordinary copies
  inference-tensor weights            a module runs its own forward (such a tensor has no ``_version``: a write could not be
                                      seen, a table would have to be packed on every call); a functional form packs on every
                                      call, stores nothing and so follows an in-place write
  autocast                            a module runs its own forward and returns autocast's dtypes; a functional form computes
                                      in float32 regardless

Every ``*_TORCH_FASTER`` / ``*_SPLIT_BELOW`` table is empty while a test runs, so a call that may take the kernels takes them
(in the tiled form) at these sizes of 5 or 6 frames.

Where two runs of a torch op chain are compared on the GPU they are held to 1e-3 of the rms, not to the bit (torch's convolutions
need not return the same bits from one algorithm choice to the next): two float32 evaluations of sums of at most 512 * 31 terms
agree to about 1e-5 of the rms, and the effect looked for, an in-place ``weight.mul_(-1.5)``, is asserted to move the result by
more than 1e-2 of it.  On the emulator leg everything runs on the CPU and is held to the bit."""
import numpy as np
import pytest
import torch

from ddsp_svc_amd import _modules as M
from ddsp_svc_amd import attention as AT
from ddsp_svc_amd import conformer as CF
from ddsp_svc_amd import naive_v2 as NV
from ddsp_svc_amd import nsf_generator as NG
from ddsp_svc_amd import wavenet as WN
from tests import attention_standin as AS
from tests import conformer_standin as CS
from tests import generator_standin as GS
from tests import naive_v2_standin as NS
from tests import wavenet_standin as WS
from tests.backends import BACKENDS, dev  # noqa: F401

FRAMES = 5
GEN_FRAMES = 6
WRITE = -1.5                                            # the in-place write of the cache tests: weight.mul_(-1.5)
MOVED = 1e-2                                            # of the rms: what that write must move a result by, at the least
TORCH_RERUN = 1e-3                                      # of the rms: two runs of one float32 torch chain on the GPU (docstring)

_TABLES = ((CF, ("CONV_TORCH_FASTER",)), (AT, ("ATTN_TORCH_FASTER",)), (WN, ("LAYER_TORCH_FASTER", "SPLIT_BELOW")),
           (NV, ("LAYER_TORCH_FASTER", "SPLIT_BELOW")), (NG, ("TORCH_FASTER", "SEAM_TORCH_FASTER", "HEAD_TORCH_FASTER")))


@pytest.fixture(autouse=True)
def every_size_routed_to_the_kernels(monkeypatch):
    """the measured tables empty and both caches empty, before and after"""
    for mod, names in _TABLES:
        for name in names:
            monkeypatch.setattr(mod, name, {})
    M.clear_packed()
    M._STACKED.clear()
    yield
    M.clear_packed()
    M._STACKED.clear()


# ---- the cases: a stand-in, its inputs, its dispatcher, its own forward ---------------------------------------------------------

def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _seeded(make, seed, gain=3.0):
    """a stand-in with torch's default initialisation under ``seed``, every weight matrix times ``gain``: the default leaves a
    conv branch at a few per cent of the x it is added to"""
    torch.manual_seed(seed)
    m = make()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.mul_(gain)
    return m


def _self_own(m, x):
    """``SelfAttention._reference_forward`` without context, mask or local heads, the inner attention as its op chain: no
    dispatcher anywhere"""
    b, n, _ = x.shape
    q, k, v = (lin(x).reshape(b, n, m.heads, -1).permute(0, 2, 1, 3) for lin in (m.to_q, m.to_k, m.to_v))
    out = AS.torch_chain(q, k, v, m.fast_attention.projection_matrix, AS.FLAG_PCMER_NORM)
    return m.dropout(m.to_out(out.permute(0, 2, 1, 3).reshape(b, n, -1)))


def _gen_inputs():
    mel, f0, source = GS.seeded_inputs("b", 2, GEN_FRAMES)
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in (mel, f0, source)]


def _gen_call(gen, mel, f0, source):
    gen.m_source.value = source
    return NG.generator_forward(gen, mel, f0)


def _gen_own(gen, mel, f0, source):
    gen.m_source.value = source
    return gen(mel, f0)


class Case:
    """``make()``: the stand-in on the CPU; ``inputs()``: its inputs on the CPU; ``call``: the dispatcher; ``own``: the module's
    own forward, no dispatcher in it; ``hip`` / ``ref``: what ONE call adds to ``hook.CALLS`` on the kernels / on the module's
    forward (every counter not named stays); ``packs``: the tables the first call on the kernels builds (None: the hook has no
    such counter); ``last``: the tensors the write goes to, the last projection among them"""

    def __init__(self, name, hook, make, inputs, call, own, hip, ref, packs, last):
        self.name, self.hook, self.make, self._inputs, self.call, self.own = name, hook, make, inputs, call, own
        self.hip, self.ref, self.packs, self.last = hip, ref, packs, last

    def module(self, device, requires_grad=False):
        m = self.make().eval().to(device)
        for p in m.parameters():
            p.requires_grad_(requires_grad)
        return m

    def inputs(self, device):
        return [t.to(device) for t in self._inputs()]

    def counts(self):
        return dict(self.hook.CALLS)

    def delta(self, before):
        return {k: v - before[k] for k, v in self.hook.CALLS.items() if v != before[k]}

    def built(self):
        return None if self.packs is None else self.hook.PACKS["count"]


_X = lambda: [_randn(11, 2, FRAMES, 256)]                                               # noqa: E731
_WN_LAYER = lambda: [_randn(21, 1, 384, FRAMES), _randn(22, 1, 256, FRAMES), 0.5 * _randn(23, 1, 384)]      # noqa: E731
_WN_NET = lambda: [_randn(24, 1, 1, 8, FRAMES), torch.tensor([40.0]), _randn(25, 1, 256, FRAMES)]           # noqa: E731
_NV_LAYER = lambda: [_randn(31, 1, 512, FRAMES), _randn(32, 1, 128, FRAMES), 0.5 * _randn(33, 1, 512, 1)]  # noqa: E731
_NV_NET = lambda: [_randn(34, 1, 8, FRAMES), torch.tensor([40.0]), _randn(35, 1, 128, FRAMES)]              # noqa: E731

CASES = [
    Case("conformer-conv", CF, lambda: _seeded(lambda: CS.ConvModule(256), 1), _X, CF.conv_forward, lambda m, x: m.net(x),
         {"hip": 1}, {"reference": 1}, 1, lambda m: [m.net[6].weight]),
    Case("conformer-layer", CF, lambda: _seeded(lambda: CS.EncoderLayer(256), 2), _X, CF.layer_forward,
         lambda m, x: x + m.conformer.net(x), {"hip": 1}, {"reference": 1}, 1, lambda m: [m.conformer.net[6].weight]),
    Case("attention-fast", AT, lambda: AS.FastAttention(), lambda: [_randn(12 + i, 1, 8, FRAMES, 64) for i in range(3)],
         AT.fast_forward, lambda m, q, k, v: m._reference_forward(q, k, v), {"hip": 1}, {"reference": 1}, 1,
         lambda m: [m.projection_matrix]),
    # the module's own forward calls the inner FastAttention, whose dispatcher counts for itself: 1 + 1
    # (gain 1: at 3 the keys' exp() leaves float16's range in the module's OWN forward under float16 autocast)
    Case("attention-self", AT, lambda: _seeded(lambda: AS.SelfAttention(256), 3, 1.0), _X, AT.self_forward, _self_own,
         {"hip": 1}, {"reference": 2}, 2, lambda m: [m.to_v.weight, m.to_out.weight]),
    Case("wavenet-layer", WN, lambda: _seeded(lambda: WS.ResidualBlock(256, 384), 4), _WN_LAYER, WN.layer_forward,
         lambda m, *a: m.reference_forward(*a), {"hip": 1}, {"reference": 1}, 1, lambda m: [m.output_projection.weight]),
    # a net's dispatcher has no counter of its own: its two layers count
    Case("wavenet-net", WN, lambda: _seeded(lambda: WS.WaveNet(in_dims=8, n_layers=2, n_chans=384, n_hidden=256), 5, 2.0),
         _WN_NET, WN.net_forward, lambda m, *a: m.reference_forward(*a), {"hip": 2}, {"reference": 2}, 2,
         lambda m: [m.residual_layers[-1].output_projection.weight, m.residual_layers[-1].diffusion_projection.weight]),
    Case("naive_v2-layer", NV, lambda: _seeded(lambda: NS.DiffLayer(512, 128), 6), _NV_LAYER, NV.layer_forward,
         lambda m, *a: m.reference_forward(*a), {"hip": 1}, {"reference": 1}, 1, lambda m: [m.conformer.net[6].weight]),
    Case("naive_v2-net", NV, lambda: _seeded(lambda: NS.Diff(8, 512, 128, num_layers=2), 7, 2.0), _NV_NET, NV.net_forward,
         lambda m, *a: m.plain_forward(*a), {"hip": 2}, {"reference": 2}, 2,
         lambda m: [m.residual_layers[-1].conformer.net[6].weight, m.residual_layers[-1].diffusion_step_projection.weight]),
    # topology "b": six blocks, two seams and the head, nothing left to torch; the head's kernel reads no table
    Case("generator", NG, lambda: GS.build("b"), _gen_inputs, _gen_call, _gen_own, {"hip": 6, "seam_hip": 2, "head_hip": 1},
         {"reference": 6, "seam_reference": 2, "head_reference": 1}, None,
         lambda m: [m.resblocks[-1].convs2[-1].weight, m.conv_post.weight]),
]
_BY_CASE = pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
_BY_DEV = pytest.mark.parametrize("dev", BACKENDS, indirect=True)


def _tup(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def _flat(r):
    return torch.cat([t.detach().float().reshape(-1) for t in _tup(r)])


def _rms(r):
    return float(_flat(r).double().pow(2).mean().sqrt())


def _same_bits(a, b):
    a, b = _tup(a), _tup(b)
    return len(a) == len(b) and all(s.dtype == t.dtype and torch.equal(s, t) for s, t in zip(a, b))


def _moved(a, b):
    """b is further from a than ``MOVED`` of a's rms"""
    return float((_flat(a) - _flat(b)).abs().max()) > MOVED * _rms(a)


def _is_own(got, want, device, rerun=TORCH_RERUN):
    """``got`` is what the module's own forward gave as ``want``: the dtypes, the shapes, finite; the bits on the CPU; on the
    GPU ``rerun`` of the rms (None: not compared)"""
    got, want = _tup(got), _tup(want)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and bool(torch.isfinite(g).all())
    if device.type == "cpu":
        assert _same_bits(got, want)
    elif rerun is not None:
        assert float((_flat(got) - _flat(want)).abs().max()) <= rerun * _rms(want)


def _cached():
    return [e[1] for e in M._PACKED.values()] + [t for e in M._STACKED.values() for t in e[1:3]]


# ---- 1. ordinary weights, the call inside inference_mode --------------------------------------------------------------------------

@_BY_DEV
@_BY_CASE
@pytest.mark.parametrize("unfrozen", [False, True], ids=["frozen", "unfrozen"])
def test_call_inside_inference_mode_takes_the_kernels_and_caches(dev, case, unfrozen):
    """The kernels run, the second call packs nothing, and a third call OUTSIDE the mode under ``no_grad`` finds the tables and
    the stacked projection that were made inside it: the same objects, the same bits.  An unfrozen model (``requires_grad``)
    is no different inside the mode, where no gradient is recorded."""
    m, inp = case.module(dev, unfrozen), case.inputs(dev)
    with torch.inference_mode():
        before, built = case.counts(), case.built()
        first = case.call(m, *inp)
        assert case.delta(before) == case.hip
        if built is not None:
            assert case.built() - built == case.packs
        kept, built, before = _cached(), case.built(), case.counts()
        assert kept and all(t.is_inference() for t in kept)
        second = case.call(m, *inp)
        assert case.delta(before) == case.hip and case.built() == built
    with torch.no_grad():
        before = case.counts()
        third = case.call(m, *inp)
        assert case.delta(before) == case.hip and case.built() == built
    again = _cached()
    assert len(again) == len(kept) and all(a is b for a, b in zip(again, kept))
    assert _same_bits(first, second) and _same_bits(first, third)
    assert all(not t.requires_grad for t in _tup(third))


# ---- 2. inference tensors as inputs -----------------------------------------------------------------------------------------------

@_BY_DEV
@_BY_CASE
def test_inference_tensor_inputs_outside_the_mode(dev, case):
    """what an encoder that ran under ``inference_mode`` hands on, used later under ``no_grad``: the kernels, and the bits that
    ordinary copies of the same inputs give"""
    m = case.module(dev)
    with torch.inference_mode():
        made = case.inputs(dev)
        made = [t.clone() for t in made]                # a seeded host tensor that .to() left where it was: a new one
    assert all(t.is_inference() for t in made)
    copies = [t.clone() for t in made]
    assert not any(t.is_inference() for t in copies)
    with torch.no_grad():
        before = case.counts()
        got = case.call(m, *made)
        assert case.delta(before) == case.hip
        before = case.counts()
        want = case.call(m, *copies)
        assert case.delta(before) == case.hip
    assert _same_bits(got, want) and bool(torch.isfinite(_flat(got)).all())


# ---- 3. inference tensors as weights: a module built inside the mode ------------------------------------------------------------------

@_BY_DEV
@_BY_CASE
def test_module_built_inside_inference_mode_runs_its_own_forward(dev, case):
    """Every parameter and buffer is an inference tensor: nothing raises, inside the mode or later under ``no_grad``; the call
    goes to the module's own forward (a twin with the same values in ordinary tensors takes the kernels); the result is that
    forward's, and after an in-place write to the last projection it is that forward's after the write."""
    with torch.inference_mode():
        m = case.module(dev)
    held = list(m.parameters()) + list(m.buffers())
    assert held and all(t.is_inference() for t in held)
    twin = case.module(dev)
    twin.load_state_dict(m.state_dict())
    inp = case.inputs(dev)
    with torch.no_grad():
        want = case.own(twin, *inp)
        before = case.counts()
        case.call(twin, *inp)
        assert case.delta(before) == case.hip           # the same values in ordinary tensors: the kernels
    M.clear_packed()
    M._STACKED.clear()

    def both_ways(want):
        for mode in (torch.inference_mode, torch.no_grad):
            with mode():
                before = case.counts()
                got = case.call(m, *inp)
                assert case.delta(before) == case.ref, mode
            _is_own(got, want, dev)
            yield got
    for got in both_ways(want):
        pass
    with torch.inference_mode():
        for t in case.last(m):
            t.mul_(WRITE)
    with torch.no_grad():
        for t in case.last(twin):
            t.mul_(WRITE)
        after = case.own(twin, *inp)
    assert _moved(want, after)                          # on the module's own forward: the write is large enough to show
    for got in both_ways(after):
        assert _moved(want, got)
    assert not M._PACKED and not M._STACKED


# ---- 4. inference tensors as weights: the functional forms ----------------------------------------------------------------------------

def _t(arrays, device):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def _params(spec_tensors):
    return [t.detach() for t in spec_tensors]


def _conv_weights(device):
    m = _seeded(lambda: CS.ConvModule(256, use_norm=True), 41).to(device)
    weights, norm, _, _ = CF._conv_spec(m)
    return _params(list(weights) + list(norm))


def _self_weights(device):
    m = _seeded(lambda: AS.SelfAttention(256), 42).to(device)
    return _params([t for lin in (m.to_q, m.to_k, m.to_v, m.to_out) for t in (lin.weight, lin.bias)]
                   + [m.fast_attention.projection_matrix])


def _wn_weights(device, layers):
    out = []
    for i in range(layers):
        weights, proj = WN._layer_spec(_seeded(lambda: WS.ResidualBlock(256, 384), 43 + i).to(device))
        out += _params(list(weights) + list(proj))
    return out


def _nv_weights(device, layers):
    out = []
    for i in range(layers):
        weights, proj = NV._layer_spec(_seeded(lambda: NS.DiffLayer(512, 128), 45 + i).eval().to(device))
        out += _params(list(weights) + list(proj))
    return out


def _by(w, n):
    return [w[i:i + n] for i in range(0, len(w), n)]


_GW = {}


def _gen_weights():
    if not _GW:
        _GW.update(GS.weights("b"))
    return _GW


class Form:
    """a functional form: ``weights(device)`` its flat list of weight tensors, ``inputs()``, ``run(w, *inputs)``; ``hook`` and
    ``packs``: the tables one call with uncached weights builds (None: no counter); ``written``: where the write goes"""

    def __init__(self, name, hook, weights, inputs, run, packs, written):
        self.name, self.hook, self.weights, self._inputs, self.run, self.packs, self.written = (name, hook, weights, inputs, run,
                                                                                               packs, written)

    def inputs(self, device):
        return [t.to(device) for t in self._inputs()]

    def built(self):
        return None if self.packs is None else self.hook.PACKS["count"]


FORMS = [
    Form("conv_module", CF, _conv_weights, _X, lambda w, x: CF.conv_module(x, w[:6], norm=(w[6], w[7])), 1, [4, 6]),
    Form("fast_attention", AT, lambda d: [AS.FastAttention().projection_matrix.to(d)],
         lambda: [_randn(12 + i, 1, 8, FRAMES, 64) for i in range(3)], lambda w, q, k, v: AT.fast_attention(q, k, v, w[0]), 1, [0]),
    Form("self_attention", AT, _self_weights, _X, lambda w, x: AT.self_attention(x, *w, heads=8), 2, [4, 6]),
    Form("residual_layer", WN, lambda d: _wn_weights(d, 1)[:6], _WN_LAYER, lambda w, x, c, s: WN.residual_layer(x, c, s, w), 1, [4]),
    Form("residual_stack", WN, lambda d: _wn_weights(d, 2), _WN_LAYER,
         lambda w, x, c, s: WN.residual_stack(x, c, s, [(l[:6], (l[6], l[7])) for l in _by(w, 8)]), 2, [12, 14]),
    Form("diff_layer", NV, lambda d: _nv_weights(d, 1)[:8],
         lambda: [_randn(31, 1, FRAMES, 512), _randn(32, 1, FRAMES, 128), 0.5 * _randn(33, 1, 512)],
         lambda w, x, c, s: NV.diff_layer(x, c, s, w), 1, [6]),
    Form("diff_stack", NV, lambda d: _nv_weights(d, 2),
         lambda: [_randn(31, 1, FRAMES, 512), _randn(32, 1, FRAMES, 128), 0.5 * _randn(33, 1, 512)],
         lambda w, x, c, s: NV.diff_stack(x, c, s, [(l[:8], (l[8], l[9])) for l in _by(w, 10)]), 2, [16, 18]),
    # (Cout, u, s) = (32, 4, 1), its three-pair k = 3 block and the 32-channel head, with topology "b"'s seeded weights
    Form("resblock1", NG, lambda d: _t([a for pair in _gen_weights()["blocks"][1][0][0] for a in pair], d),
         lambda: [_randn(51, 2, 32, FRAMES)], lambda w, x: NG.resblock1(x, _by(w, 4), GS.DILATIONS), None, [10]),
    Form("upsample_stage", NG, lambda d: _t(_gen_weights()["seams"][1], d),
         lambda: [_randn(52, 2, 64, FRAMES), 0.5 * _randn(53, 2, 1, 4 * FRAMES)],
         lambda w, x, src: NG.upsample_stage(x, w[0], w[1], 4, src, w[2], w[3], 1), None, [0]),
    Form("output_head", NG, lambda d: _t(_gen_weights()["head"], d), lambda: [_randn(54, 2, 32, FRAMES)],
         lambda w, x: NG.output_head(x, w[0], w[1]), None, [0]),
]
_BY_FORM = pytest.mark.parametrize("form", FORMS, ids=[f.name for f in FORMS])


@_BY_DEV
@_BY_FORM
def test_functional_forms_with_inference_tensor_weights(dev, form):
    """No module to hand the call to: the kernels run, on a table packed on EVERY call and stored nowhere, so the result is the
    one ordinary clones of the weights give -- before an in-place write inside the mode and after it."""
    plain, inp = form.weights(dev), form.inputs(dev)
    with torch.inference_mode():
        held = [t.clone() for t in plain]
    assert all(t.is_inference() for t in held) and not any(t.is_inference() for t in plain)

    def every_call_packs(want):
        M.clear_packed()
        M._STACKED.clear()
        for mode in (torch.inference_mode, torch.no_grad):
            with mode():
                built = form.built()
                got = form.run(held, *inp)
            assert _same_bits(got, want), mode
            assert built is None or form.built() - built == form.packs
            assert not M._PACKED and not M._STACKED
    with torch.no_grad():
        want = form.run(plain, *inp)
    assert bool(torch.isfinite(_flat(want)).all())
    every_call_packs(want)
    with torch.inference_mode():
        for i in form.written:
            held[i].mul_(WRITE)
    with torch.no_grad():
        after = form.run([t.clone() for t in held], *inp)
    assert _moved(want, after)
    every_call_packs(after)


# ---- 5. autocast ----------------------------------------------------------------------------------------------------------------------

_AUTOCAST = [pytest.param("emu", torch.bfloat16, id="emu-bfloat16"),
             pytest.param("gpu", torch.bfloat16, id="gpu-bfloat16", marks=pytest.mark.gpu),
             pytest.param("gpu", torch.float16, id="gpu-float16", marks=pytest.mark.gpu)]
_BY_AUTOCAST = pytest.mark.parametrize("dev, dtype", _AUTOCAST, indirect=["dev"])


@_BY_AUTOCAST
@_BY_CASE
def test_under_autocast_a_module_runs_its_own_forward(dev, dtype, case):
    """No hook raises; the call goes to the module's own forward -- the inner ``FastAttention`` of a ``SelfAttention`` and the
    conv module of an ``EncoderLayer`` as well: no kernel counter moves -- and has the dtypes that forward returns under the same
    autocast.  A nested ``autocast(enabled=False)``, and an autocast for another device type, keep the kernels and the bits of
    the plain call."""
    m, inp = case.module(dev), case.inputs(dev)
    with torch.no_grad():
        before = case.counts()
        plain = case.call(m, *inp)
        assert case.delta(before) == case.hip
        with torch.autocast(dev.type, dtype=dtype):
            want = case.own(m, *inp)
            before = case.counts()
            got = case.call(m, *inp)
            assert case.delta(before) == case.ref
            _is_own(got, want, dev, rerun=None)
            with torch.autocast(dev.type, enabled=False):
                before = case.counts()
                nested = case.call(m, *inp)
                assert case.delta(before) == case.hip
        assert _same_bits(nested, plain)
        if dev.type != "cpu":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                before = case.counts()
                other = case.call(m, *inp)
                assert case.delta(before) == case.hip
            assert _same_bits(other, plain)


@_BY_AUTOCAST
def test_under_autocast_the_generators_lines_run_the_torch_lines(dev, dtype):
    """a block, a seam and the head, each handed a float32 boundary inside an autocast region (``generator_forward`` hands them
    ``conv_pre``'s half-precision one, which no kernel would take anyway): the torch line, in its dtype"""
    gen = GS.build("b", dev)
    x0, x1, src = [t.to(dev) for t in (_randn(61, 2, 128, FRAMES), _randn(62, 2, 64, 8 * FRAMES), 0.5 * _randn(63, 2, 1, 32 * FRAMES))]
    lines = [(lambda: NG.resblock_forward(gen.resblocks[0], x1), lambda: gen.resblocks[0].chain(x1), "hip", "reference"),
             (lambda: NG.seam_forward(gen.ups[0], gen.noise_convs[0], x0, src), lambda: gen.torch_seam(0, x0, src),
              "seam_hip", "seam_reference"),
             (lambda: NG.head_forward(gen.conv_post, x1[:, :32]), lambda: gen.torch_head(x1[:, :32]), "head_hip", "head_reference")]
    with torch.no_grad():
        for call, own, hip, ref in lines:
            before = dict(NG.CALLS)
            plain = call()
            assert {k: v - before[k] for k, v in NG.CALLS.items() if v != before[k]} == {hip: 1}
            with torch.autocast(dev.type, dtype=dtype):
                want = own()
                before = dict(NG.CALLS)
                got = call()
                assert {k: v - before[k] for k, v in NG.CALLS.items() if v != before[k]} == {ref: 1}
                _is_own(got, want, dev, rerun=None)
                with torch.autocast(dev.type, enabled=False):
                    assert _same_bits(call(), plain)


@_BY_AUTOCAST
@_BY_FORM
def test_functional_forms_compute_in_float32_inside_autocast(dev, dtype, form):
    """float32 in, float32 out, the bits of the call outside the region"""
    w, inp = form.weights(dev), form.inputs(dev)
    with torch.no_grad():
        want = form.run(w, *inp)
        with torch.autocast(dev.type, dtype=dtype):
            got = form.run(w, *inp)
    assert all(t.dtype == torch.float32 for t in _tup(got)) and _same_bits(got, want)


# ---- 6. the drop-in harmonic source ---------------------------------------------------------------------------------------------------

@_BY_DEV
def test_source_module_in_every_mode(dev, monkeypatch):
    """``nsf_source.SourceModuleHnNSF`` with identical draws: inside ``inference_mode``, under bfloat16 autocast and in a plain
    ``no_grad`` call it returns the same float32 bits"""
    from oracle import ddsp_oracle as O
    from ddsp_svc_amd import nsf_source as S
    sr, upp = 44100, 512
    m = S.SourceModuleHnNSF(sr, harmonic_num=8).to(dev)
    f0 = torch.from_numpy(O.synth_f0(2, FRAMES, sr, upp, seed=1)[..., 0]).to(dev)
    ri = torch.rand(1, 1, 9, generator=torch.Generator().manual_seed(2)).to(dev)
    nz = torch.randn(2, FRAMES * upp, 9, generator=torch.Generator().manual_seed(3)).to(dev)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: ri.clone())
    monkeypatch.setattr(torch, "randn", lambda *a, **k: nz)
    with torch.no_grad():
        plain = m(f0, upp)
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            cast = m(f0, upp)
    with torch.inference_mode():
        inside = m(f0, upp)
    assert plain.shape == (2, FRAMES * upp, 1) and plain.dtype == torch.float32 and bool(torch.isfinite(plain).all())
    assert float(plain.abs().max()) > 0.01
    assert _same_bits(cast, plain) and _same_bits(inside, plain)


# ---- the one place that reads a version ---------------------------------------------------------------------------------------------

def test_versions_of_is_none_for_a_key_with_an_inference_tensor():
    a, b = torch.zeros(3), torch.zeros(3)
    with torch.inference_mode():
        c = torch.zeros(3)
    assert M.tracked(a, None, b) and not M.tracked(a, c) and M.tracked()
    assert M.versions_of([a, b]) == (0, 0) and M.versions_of([a, c]) is None
    a.add_(1)
    assert M.versions_of([a, b]) == (1, 0)
    for conv in (torch.nn.Conv1d(4, 8, 1), torch.nn.Linear(4, 4)):
        assert M.plain(conv) and M.plain_with_bias(conv)
    with torch.inference_mode():
        built = torch.nn.Conv1d(4, 8, 1)
        bias = torch.nn.Parameter(torch.zeros(8))
    assert not M.plain(built) and not M.plain_with_bias(built) and not M.pointwise(built, 4, 8)
    mixed = torch.nn.Conv1d(4, 8, 1)
    mixed.bias = bias                                   # an ordinary weight, a bias from inside the mode
    assert not M.plain(mixed) and not M.plain_with_bias(mixed)
    assert M.plain(torch.nn.Conv1d(4, 8, 1, bias=False))
