"""The conformer conv module (ddsp_svc_amd.conformer, csrc/conformer_conv.h): the HIP kernel on the emulator and the GPU against the
float64 oracle, the zero-padded intermediate, the GLU halves and tap orientation, the LayerNorm, the encoder, the batch split, the
C ABI, the dispatch and the reference hook.

The parity bar is test_resblock.py's, relative to what float32 itself does on the same inputs: with e_torch = max|the torch op
chain in float32 on the CPU - oracle|, the kernel must stay within 4 e_torch + 1e-7 rms(oracle) (another summation order over 256
and 512 terms).  Every case prints its err / bar."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conformer_oracle as O
from tests import conformer_standin as S
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import _ffi, conformer as CF  # noqa: E402

D = 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conformer_conv.npz")
NAMES = ("w1", "b1", "wd", "bd", "w2", "b2")
NAN = float("nan")


SHIPPED_TORCH_FASTER = dict(CF.CONV_TORCH_FASTER)


@pytest.fixture(autouse=True)
def _structural_dispatch(monkeypatch):
    """the dispatch tests decide from a module's structure at shapes of a few frames: the measured crossover table (whose own
    test reads SHIPPED_TORCH_FASTER) is empty while they run, as it is in tools/conformer_bench.py"""
    monkeypatch.setattr(CF, "CONV_TORCH_FASTER", {})


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def test_crossover_table_agrees_with_the_committed_measurements():
    """every module case of profiles/conformer_{throughput,latency}.json is routed to whichever side was measured faster"""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = []
    for mode in ("throughput", "latency"):
        with open(os.path.join(root, "profiles", "conformer_%s.json" % mode)) as f:
            doc = json.load(f)
        assert doc["D"] == D and doc["tile"] == 98
        cases += [c for c in doc["cases"] if c["case"].startswith("module")]
    assert {c["frames"] for c in cases} == {100, 203, 48 * 172, 32 * 862}
    for c in cases:
        to_torch = D in SHIPPED_TORCH_FASTER and (SHIPPED_TORCH_FASTER[D] is None or c["frames"] < SHIPPED_TORCH_FASTER[D])
        assert to_torch == (c["torch_over_hip"] < 1.0), (c["case"], c["frames"], c["torch_over_hip"], SHIPPED_TORCH_FASTER)


def _torch_chain(x, weights, norm=None, eps=1e-5, add_input=False):
    """the module's op chain as torch ops in float32 on the CPU"""
    x = torch.as_tensor(x)
    w1, b1, wd, bd, w2, b2 = [torch.as_tensor(a) for a in weights]
    h = x if norm is None else F.layer_norm(x, (x.shape[-1],), torch.as_tensor(norm[0]), torch.as_tensor(norm[1]), eps)
    h = F.glu(F.conv1d(h.transpose(1, 2), w1, b1), dim=1)
    h = F.silu(F.conv1d(h, wd, bd, padding=wd.shape[-1] // 2, groups=wd.shape[0]))
    y = F.conv1d(h, w2, b2).transpose(1, 2)
    return (x + y if add_input else y).numpy()


def _bar(x, weights, ref, norm=None, eps=1e-5, add_input=False):
    e_torch = float(np.abs(_torch_chain(x, weights, norm, eps, add_input).astype(np.float64) - ref).max())
    return 4.0 * e_torch + 1e-7 * _rms(ref), e_torch


def _t(arrays, device):
    """tensors of their own: an in-place write to one must not reach the numpy arrays the oracle reads"""
    return None if arrays is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).clone().to(device) for a in arrays)


def _run(x, wt, device, **kw):
    return CF.conv_module(torch.from_numpy(x).to(device), wt, **kw).cpu().numpy().astype(np.float64)


# ---- the oracle against the reference's own output ------------------------------------------------------------------------------

def test_oracle_matches_reference_fixture():
    g = np.load(GOLDEN)
    x = g["x"]
    assert x.shape == (2, 70, 32)
    for tag in ("plain", "norm"):
        weights = tuple(g["%s_%s" % (tag, n)] for n in NAMES)
        norm = (g["norm_gamma"], g["norm_beta"]) if tag == "norm" else None
        want = O.net(x, weights, norm)
        assert _rms(want) > 0.5 * _rms(x)              # the conv terms are of x's size, not vanishing
        assert np.abs(g[tag + "_y"] - want).max() <= 1e-5 * _rms(want)
        assert np.abs(_torch_chain(x, weights, norm) - g[tag + "_y"]).max() <= 1e-5 * _rms(want)
    layers = [(tuple(g["enc%d_%s" % (i, n)] for n in NAMES), None, 1e-5) for i in range(3)]
    want = O.encoder(x, layers)
    assert _rms(O.net(x, layers[0][0])) > 0.5 * _rms(x)
    assert np.abs(g["enc_y"] - want).max() <= 1e-5 * _rms(want)


def test_seeded_weights_keep_the_conv_terms_at_the_size_of_x():
    x = np.random.default_rng(0).standard_normal((1, 64, D)).astype(np.float32)
    for w, norm in ((O.seeded_weights(D, 1), None), (O.seeded_weights(D, 2), O.seeded_norm(D, 3))):
        assert 0.5 < _rms(O.net(x, w, norm)) < 2.0


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("add_input", [False, True], ids=["net", "residual"])
@pytest.mark.parametrize("use_norm", [False, True], ids=["plain", "norm"])
def test_parity(dev, use_norm, add_input):
    t = CF.tile(D)
    assert t == 98
    weights = O.seeded_weights(D, 10 + use_norm)
    norm = O.seeded_norm(D, 12) if use_norm else None
    wt, nt = _t(weights, dev), _t(norm, dev)
    rng = np.random.default_rng(2 * use_norm + add_input)
    worst = 0.0
    for L in (1, 15, 16, 31, t - 1, t, t + 1, 2 * t + 17):
        x = rng.standard_normal((2, L, D)).astype(np.float32)
        assert not np.array_equal(x[0], x[1])
        ref = O.net(x, weights, norm) + (x if add_input else 0.0)
        bar, e_torch = _bar(x, weights, ref, norm, add_input=add_input)
        y = _run(x, wt, dev, norm=nt, add_input=add_input)
        err = float(np.abs(y - ref).max())
        print("norm %d add %d L %d: hip %.3e torch %.3e bar %.3e err / bar %.3f" % (use_norm, add_input, L, err, e_torch, bar,
                                                                                      err / bar))
        worst = max(worst, err / bar)
        assert err <= bar, (L, err, bar, e_torch)
    print("worst err / bar %.3f" % worst)


# ---- edges: the depthwise conv pads its own input -------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_intermediate_is_zero_outside_the_sequence(dev):
    t = CF.tile(D)
    weights = O.seeded_weights(D, 20, bias_std=1.0)
    wt = _t(weights, dev)
    rng = np.random.default_rng(21)
    for L in (1, t + 1):
        x = rng.standard_normal((2, L, D)).astype(np.float32)
        ref = O.net(x, weights)
        bar, _ = _bar(x, weights, ref)
        err = float(np.abs(_run(x, wt, dev) - ref).max())
        print("L %d: err / bar %.3f" % (L, err / bar))
        assert err <= bar, (L, err, bar)
        wrong = O.net(x, weights, halo_from_padded_x=True)
        assert np.abs(wrong - ref).max() > 100 * bar, (L, np.abs(wrong - ref).max(), bar)   # the case can fail


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_glu_halves_and_tap_orientation(dev):
    weights = O.seeded_weights(D, 30, asymmetric=True)
    x = np.random.default_rng(31).standard_normal((2, 40, D)).astype(np.float32)
    ref = O.net(x, weights)
    bar, _ = _bar(x, weights, ref)
    err = float(np.abs(_run(x, _t(weights, dev), dev) - ref).max())
    print("err / bar %.3f" % (err / bar))
    assert err <= bar
    assert np.abs(O.net(x, weights, swap_glu=True) - ref).max() > 100 * bar
    assert np.abs(O.net(x, weights, flip_taps=True) - ref).max() > 100 * bar


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_layer_norm_edges(dev):
    """frame 0: all channels equal (variance 0: the result rests on eps); frame 1: mean 1e3 (a one-pass variance E[x^2] - E[x]^2
    cancels in float32); a non-default eps"""
    weights, norm, eps = O.seeded_weights(D, 40), O.seeded_norm(D, 41), 0.1       # 5 % off the default's 1 / sqrt(var + 1e-5)
    rng = np.random.default_rng(42)
    x = rng.standard_normal((2, 5, D)).astype(np.float32)
    x[:, 0, :] = np.float32(0.37)
    x[1, 0, :] = np.float32(-2.5)
    x[:, 1, :] = (1e3 + rng.standard_normal((2, D))).astype(np.float32)
    ref = O.net(x, weights, norm, eps)
    bar, e_torch = _bar(x, weights, ref, norm, eps)
    y = _run(x, _t(weights, dev), dev, norm=_t(norm, dev), eps=eps)
    assert np.isfinite(y).all()
    err = float(np.abs(y - ref).max())
    print("hip %.3e torch %.3e err / bar %.3f" % (err, e_torch, err / bar))
    assert err <= bar
    assert np.abs(O.net(x, weights, norm, 1e-5) - ref).max() > 100 * bar          # eps is not ignored
    one_pass = x.astype(np.float32)                                                # the cancellation the case is about
    var1 = (one_pass[:, 1] ** 2).mean(-1, dtype=np.float32) - one_pass[:, 1].mean(-1, dtype=np.float32) ** 2
    var2 = x[:, 1].astype(np.float64).var(-1)
    assert np.abs(var1 - var2).max() > 1e-2 * var2.max()


# ---- the encoder and the packed cache -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_encoder_and_packed_cache(dev):
    layers = [(O.seeded_weights(D, 50 + i), O.seeded_norm(D, 60) if i == 1 else None, 1e-5) for i in range(3)]
    lt = [(_t(w, dev), _t(n, dev), e) for w, n, e in layers]
    x = np.random.default_rng(51).standard_normal((2, 20, D)).astype(np.float32)
    xt = torch.from_numpy(x).to(dev)

    def ref_and_bar():
        ref = O.encoder(x, layers)
        chain = x
        for w, n, e in layers:
            chain = _torch_chain(chain, w, n, e, add_input=True)
        return ref, 4.0 * float(np.abs(chain.astype(np.float64) - ref).max()) + 1e-7 * _rms(ref)

    ref, bar = ref_and_bar()
    p0 = CF.PACKS["count"]
    y = CF.encoder(xt, lt)
    assert CF.PACKS["count"] == p0 + 3
    assert torch.equal(xt.cpu(), torch.from_numpy(x))                             # x is never written
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print("encoder err / bar %.3f" % (err / bar))
    assert err <= bar
    step = xt
    for w, n, e in lt:
        step = CF.conv_module(step, w, norm=n, eps=e, add_input=True)
    assert torch.equal(step, y)                                                   # bit for bit
    out = torch.full_like(xt, NAN)
    assert CF.encoder(xt, lt, out=out) is out and torch.equal(out, y)
    assert CF.PACKS["count"] == p0 + 3                                            # every later call found the cached tables
    with pytest.raises(ValueError):
        CF.encoder(xt, lt, out=xt)
    with pytest.raises(ValueError):
        CF.conv_module(xt, lt[0][0], out=xt)
    # an in-place write bumps _version: one table is rebuilt and the result follows the new weight
    lt[2][0][4].mul_(-1.5)
    layers[2] = (tuple(a if i != 4 else (a * np.float32(-1.5)) for i, a in enumerate(layers[2][0])), None, 1e-5)
    y2 = CF.encoder(xt, lt)
    assert CF.PACKS["count"] == p0 + 4
    ref2, bar2 = ref_and_bar()
    assert np.abs(ref2 - ref).max() > 100 * bar2
    assert np.abs(y2.cpu().numpy() - ref2).max() <= bar2


# ---- batch split ------------------------------------------------------------------------------------------------------------------

def _rows_differ(a):
    a = np.asarray(a).reshape(len(a), -1)
    for i in range(a.shape[0]):
        for j in range(i + 1, a.shape[0]):
            assert not np.array_equal(a[i], a[j]), (i, j)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_batch_split(dev, knobs):
    """BATCH_SPLIT 2 and 1 at B = 5: chunks 2, 2, 1 (two non-zero bases, an uneven tail) meet two column tiles"""
    L = CF.tile(D) + 1
    weights, norm = O.seeded_weights(D, 70), O.seeded_norm(D, 71)
    wt, nt = _t(weights, dev), _t(norm, dev)
    x = np.random.default_rng(72).standard_normal((5, L, D)).astype(np.float32)
    ref = O.net(x, weights, norm) + x
    bar, _ = _bar(x, weights, ref, norm, add_input=True)
    xt = torch.from_numpy(x).to(dev)
    whole = CF.conv_module(xt, wt, norm=nt, add_input=True, out=torch.full_like(xt, NAN))
    err = float(np.abs(whole.cpu().numpy() - ref).max())
    print("err / bar %.3f" % (err / bar))
    assert err <= bar
    _rows_differ(whole.cpu().numpy())
    _rows_differ(ref)
    for split in (2, 1):
        knobs("BATCH_SPLIT", split)
        part = CF.conv_module(xt, wt, norm=nt, add_input=True, out=torch.full_like(xt, NAN))
        assert torch.isfinite(part).all(), split
        assert torch.equal(part, whole), split


@pytest.mark.gpu
def test_past_the_grid_limit():
    """B = 65 537 = 65 535 + 2 at L = 4, x[b] = pool[b % 251] (251 is prime and 65 535 mod 251 = 24: a wrong base or stride moves an
    utterance onto another pool entry), compared bitwise with the pool's own run, which the oracle checks.  268 MB per tensor."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    POOL, B, L = 251, 65535 + 2, 4
    weights = O.seeded_weights(D, 80)
    wt = _t(weights, device)
    xp = np.random.default_rng(81).standard_normal((POOL, L, D)).astype(np.float32)
    ref = O.net(xp, weights) + xp
    bar, _ = _bar(xp, weights, ref, add_input=True)
    xpool = torch.from_numpy(xp).to(device)
    ypool = CF.conv_module(xpool, wt, add_input=True)
    assert float(np.abs(ypool.cpu().numpy() - ref).max()) <= bar
    _rows_differ(ref)
    idx = torch.arange(B, device=device) % POOL
    x = xpool[idx].contiguous()
    y = CF.conv_module(x, wt, add_input=True, out=torch.full_like(x, NAN))
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    assert lib.ddsp_hip_conformer_conv_tile(D) == 98
    assert [lib.ddsp_hip_conformer_conv_tile(d) for d in (512, 128, 0, -256)] == [0, 0, 0, 0]
    floats = 4 * D * D + 2 * D * D + 4 * D + 2 * D * 31 + 2 * D + D
    assert lib.ddsp_hip_conformer_conv_pack_bytes(D, 0) == 4 * floats
    assert lib.ddsp_hip_conformer_conv_pack_bytes(D, 1) == 4 * (floats + 2 * D)
    assert [lib.ddsp_hip_conformer_conv_pack_bytes(d, 0) for d in (512, 128, 0)] == [0, 0, 0]
    weights, norm = O.seeded_weights(D, 90), O.seeded_norm(D, 91)
    w = [torch.from_numpy(a) for a in weights + norm]
    need = 4 * (floats + 2 * D)
    tab = torch.zeros(need // 4)
    ptrs = [a.data_ptr() for a in w]
    pack = lambda p, d=D, n=need: lib.ddsp_hip_conformer_conv_pack(*p, d, tab.data_ptr(), n)
    assert pack(ptrs, n=need - 4) == -4
    assert pack(ptrs, d=512) == -3 and pack(ptrs, d=128) == -3
    assert pack([None] + ptrs[1:]) == -1
    assert pack(ptrs[:6] + [ptrs[6], None]) == -1      # a gamma without a beta
    assert pack(ptrs[:6] + [None, None], n=4 * floats) == 0
    assert pack(ptrs) == 0
    L = 6
    x = torch.randn(2, L, D, generator=torch.Generator().manual_seed(1))
    y = torch.full((2, L, D), 7.0)
    call = lambda **kw: lib.ddsp_hip_conformer_conv(*[kw.get(n, d) for n, d in (
        ("x", x.data_ptr()), ("y", y.data_ptr()), ("t", tab.data_ptr()), ("tb", need), ("B", 2), ("L", L), ("D", D), ("norm", 1),
        ("eps", 1e-5), ("add", 0), ("st", None))])
    for kw, code in (({"D": 128}, -3), ({"D": 512}, -3), ({"D": 0}, -3), ({"L": 0}, -1), ({"L": -1}, -1), ({"L": 2 ** 40 + 1}, -3),
                     ({"y": x.data_ptr()}, -1), ({"tb": need - 4}, -4), ({"tb": 4 * floats}, -4), ({"x": None}, -1),
                     ({"y": None}, -1), ({"t": None}, -1), ({"B": -1}, -1), ({"eps": float("nan")}, -1),
                     ({"x": x.data_ptr() + 4}, -1)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all(), kw                    # refused before any launch
    assert call(B=0, x=None, y=None) == 0 and (y == 7.0).all()                    # a no-op
    assert call(norm=0, tb=4 * floats) == 0            # without the LayerNorm the shorter table is enough
    assert call() == 0
    ref = O.net(x.numpy(), weights, norm)
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


# ---- dispatch -------------------------------------------------------------------------------------------------------------------

def _counts():
    return CF.CALLS["hip"], CF.CALLS["reference"]


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_dispatch(dev, monkeypatch):
    from ddsp_svc_amd import nsf_generator as NG
    ng_calls = dict(NG.CALLS)
    torch.manual_seed(0)
    x = torch.randn(1, 5, D)
    forms = [S.ConvModule(D), S.ConvModule(D, use_norm=True), S.ConvModule(D, pcmer=True), S.ConvModule(D, dropout=0.1).eval()]
    with torch.no_grad():
        for m in forms:                                # both depthwise forms, both GLU / SiLU spellings: the kernel
            h0, r0 = _counts()
            y = m(x)
            assert _counts() == (h0 + 1, r0)
            want = m.net(x)
            assert (y - want).abs().max() <= 1e-5 * float(want.abs().max())

        def goes_to_reference(m, xin):
            h0, r0 = _counts()
            y = m(xin)
            assert _counts() == (h0, r0 + 1)
            assert torch.equal(y, m.net(xin))

        goes_to_reference(S.ConvModule(128), torch.randn(1, 5, 128))              # dim 128
        goes_to_reference(S.ConvModule(D, taps=29), x)                            # 29 taps
        goes_to_reference(S.ConvModule(D, expansion=1), x)                        # expansion 1
        wn = S.ConvModule(D)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.nn.utils.weight_norm(wn.net[2])
        goes_to_reference(wn, x)                                                  # a weight-normed pointwise conv
        hooked = S.ConvModule(D)
        hooked.net[6].register_forward_hook(lambda mod, inp, out: None)
        goes_to_reference(hooked, x)                                              # a forward hook
        goes_to_reference(S.ConvModule(D).double(), x.double())                   # float64
        monkeypatch.setitem(CF.CONV_TORCH_FASTER, D, 6)
        goes_to_reference(forms[0], x)                                            # B L = 5 is below the measured crossover
        monkeypatch.setitem(CF.CONV_TORCH_FASTER, D, 5)
        h0, r0 = _counts()
        forms[0](x)
        assert _counts() == (h0 + 1, r0)
        monkeypatch.setitem(CF.CONV_TORCH_FASTER, D, None)
        goes_to_reference(forms[0], x)
        monkeypatch.delitem(CF.CONV_TORCH_FASTER, D)
    # train mode with an active dropout: the module's own net (seeded, so that both draws agree)
    tr = S.ConvModule(D, dropout=0.1).train()
    with torch.no_grad():
        h0, r0 = _counts()
        torch.manual_seed(5)
        y = tr(x)
        torch.manual_seed(5)
        assert torch.equal(y, tr.net(x)) and _counts() == (h0, r0 + 1)
        assert S.ConvModule(D, dropout=0.0).train()(x) is not None and _counts() == (h0 + 1, r0 + 1)   # p = 0 is inactive
    # a gradient is needed: the differentiable chain; the same module under no_grad: the kernel
    m = forms[0]
    xg = x.clone().requires_grad_(True)
    h1, r1 = _counts()
    yg = m(xg)
    assert _counts() == (h1, r1 + 1) and yg.requires_grad
    yg.sum().backward()
    assert xg.grad is not None and m.net[2].weight.grad is not None
    with torch.no_grad():
        m(xg)
        assert _counts() == (h1 + 1, r1 + 1)
    assert NG.CALLS == ng_calls                        # the generator's counters are not touched


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_layer_dispatch(dev):
    torch.manual_seed(1)
    x = torch.randn(1, 4, D)
    with torch.no_grad():
        layer = S.EncoderLayer(D)
        h0, r0 = _counts()
        y = layer(x)                                   # conv only: one launch with the residual add inside
        assert _counts() == (h0 + 1, r0)
        want = x + layer.conformer.net(x)
        assert (y - want).abs().max() <= 1e-5 * float(want.abs().max())
        att = S.EncoderLayer(D, attn=S.ScaleAttn())
        h0, r0 = _counts()
        y = att(x)                                     # the reference's two lines; the conv module dispatches for itself
        assert _counts() == (h0 + 1, r0)
        x1 = x + 0.5 * att.norm(x)
        want = x1 + att.conformer.net(x1)
        assert (y - want).abs().max() <= 1e-5 * float(want.abs().max())
        small = S.EncoderLayer(128)
        xs = torch.randn(1, 4, 128)
        h0, r0 = _counts()
        assert torch.equal(small(xs), xs + small.conformer.net(xs)) and _counts() == (h0, r0 + 1)


def test_dispatch_keeps_host_tensors_on_the_reference():
    m = S.ConvModule(D)
    x = torch.randn(1, 3, D)
    with torch.no_grad():
        h0, r0 = _counts()
        assert torch.equal(m(x), m.net(x)) and _counts() == (h0, r0 + 1)


# ---- the reference hook -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_reference_hook(dev):
    ref_root = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
    if not os.path.isdir(os.path.join(ref_root, "reflow")):
        pytest.skip("reference checkout not present (only in the build container)")
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    import reflow.model_conformer_naive as M
    conv_fwd, layer_fwd = M.ConformerConvModule.forward, M.CFNEncoderLayer.forward
    enc = M.ConformerNaiveEncoder(3, 8, D, False, True, 0, 0.1).eval()
    for i, layer in enumerate(enc.encoder_layers):     # the default initialisation would leave only the residual
        S.load(layer.conformer, O.seeded_weights(D, 100 + i))
    x = torch.randn(2, 30, D, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        want = enc(x)
        exact = enc.double()(x.double()).numpy()
        enc.float().to(dev)
        try:
            mods = CF.patch_reference_conformer()
            assert M in mods
            patched = M.ConformerConvModule.forward
            assert patched is not conv_fwd and M.CFNEncoderLayer.forward is not layer_fwd
            CF.patch_reference_conformer()             # idempotent
            assert M.ConformerConvModule.forward is patched and M.ConformerConvModule._reference_forward is conv_fwd
            h0, r0 = _counts()
            got = enc(x.to(dev))
            assert _counts() == (h0 + 3, r0)
            one = enc.encoder_layers[0].conformer(x.to(dev))                      # the module through its own forward
            assert one.shape == x.shape and _counts() == (h0 + 4, r0)
        finally:
            CF.unpatch_reference_conformer()
        assert M.ConformerConvModule.forward is conv_fwd and M.CFNEncoderLayer.forward is layer_fwd
        assert "_reference_forward" not in M.ConformerConvModule.__dict__ and "_reference_forward" not in M.CFNEncoderLayer.__dict__
    e_torch = float(np.abs(want.numpy() - exact).max())
    err = float(np.abs(got.cpu().numpy() - exact).max())
    bar = 4 * e_torch + 1e-7 * _rms(exact)
    print("encoder through the hook: hip %.3e torch %.3e err / bar %.3f" % (err, e_torch, err / bar))
    assert err <= bar


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _gui_case(device):
    weights, norm = O.seeded_weights(D, 110), O.seeded_norm(D, 111)
    x = torch.randn(1, 203, D, generator=torch.Generator().manual_seed(4)).to(device)   # the GUI's 2.35 s window
    return x, weights, norm, _t(weights, device), _t(norm, device)


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical_and_allocates_only_the_output():
    """a call is one launch on the caller's stream: a capture of it is a single node, no parallel branches"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    x, weights, norm, wt, nt = _gui_case(device)
    eager = CF.conv_module(x, wt, norm=nt, add_input=True)                          # the warm call packs the table
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(device)
    y = CF.conv_module(x, wt, norm=nt, add_input=True)
    assert torch.cuda.memory_allocated(device) - before == y.numel() * 4
    ref = O.net(x.cpu().numpy(), weights, norm) + x.cpu().numpy()
    bar, _ = _bar(x.cpu().numpy(), weights, ref, norm, add_input=True)
    assert np.abs(eager.cpu().numpy() - ref).max() <= bar
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        CF.conv_module(x, wt, norm=nt, add_input=True, out=out)
    for _ in range(2):
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.gpu
def test_gpu_non_default_stream_is_honoured():
    """x is produced on a side stream right before the call, without any synchronisation in between: only a launch on that same
    stream is ordered behind it"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    x, weights, norm, wt, nt = _gui_case(device)
    eager = CF.conv_module(x, wt, norm=nt)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    big = torch.randn(4096, 4096, device=device)
    xs = torch.zeros_like(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big @ big * 1e-2                     # keeps the side stream busy while the host runs ahead
        xs.copy_(x)
        y = CF.conv_module(xs, wt, norm=nt)
    side.synchronize()
    assert torch.equal(y, eager)
