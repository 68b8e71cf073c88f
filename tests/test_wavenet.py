"""The WaveNet residual layer (ddsp_svc_amd.wavenet, csrc/wavenet_layer.h): the HIP kernel on the emulator and the GPU against the
float64 oracle, the zero padding of x + d, the halves of z and o and the tap orientation, saturation, the stack with its running
skip sum, the batch split, the C ABI, the dispatch and the reference hook.

The parity bar is test_conformer.py's, relative to what float32 itself does on the same inputs: with e_torch = max|the torch op
chain in float32 on the CPU - oracle|, the kernel must stay within 4 e_torch + 1e-7 rms(oracle), separately for x_out and skip
(another summation order over 3 C + H and C terms).  Every case prints its err / bar."""
import json
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wavenet_oracle as O
from tests import wavenet_standin as S
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import _ffi, wavenet as WN  # noqa: E402

H = 256
SHAPES = ((384, H), (512, H))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wavenet_layer.npz")
NAMES = ("wdil", "bdil", "wc", "bc", "wo", "bo")
NAN = float("nan")

SHIPPED_TORCH_FASTER = dict(WN.LAYER_TORCH_FASTER)


@pytest.fixture(autouse=True)
def _structural_dispatch(monkeypatch):
    """the dispatch tests decide from a module's structure at shapes of a few frames: the measured crossover table (whose own
    test reads SHIPPED_TORCH_FASTER) is empty while they run, as it is in tools/wavenet_bench.py"""
    monkeypatch.setattr(WN, "LAYER_TORCH_FASTER", {})


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def _torch_layer(x, cond, d, weights):
    """the layer's op chain as torch ops in float32 on the CPU"""
    x, cond, d = [torch.as_tensor(np.asarray(a, np.float32)) for a in (x, cond, d)]
    wdil, bdil, wc, bc, wo, bo = [torch.as_tensor(a) for a in weights]
    C = x.shape[1]
    y = F.conv1d(x + d.unsqueeze(-1), wdil, bdil, padding=1) + F.conv1d(cond, wc, bc)
    gate, filt = torch.split(y, [C, C], dim=1)
    y = F.conv1d(torch.sigmoid(gate) * torch.tanh(filt), wo, bo)
    res, skip = torch.split(y, [C, C], dim=1)
    return ((x + res) / math.sqrt(2.0)).numpy(), skip.numpy()


def _torch_stack(x, cond, s, layers):
    x, s32 = np.asarray(x, np.float32), torch.as_tensor(np.asarray(s, np.float32))
    total = None
    for weights, (wp, bp) in layers:
        d = F.linear(s32, torch.as_tensor(wp), torch.as_tensor(bp)).numpy()
        x, skip = _torch_layer(x, cond, d, weights)
        total = skip if total is None else total + skip
    return x, total


def _bars(chain, ref):
    """(bar for x_out, bar for skip) from the float32 chain's own error"""
    return tuple(4.0 * float(np.abs(c.astype(np.float64) - r).max()) + 1e-7 * _rms(r) for c, r in zip(chain, ref))


def _t(arrays, device):
    """tensors of their own: an in-place write to one must not reach the numpy arrays the oracle reads"""
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).clone().to(device) for a in arrays)


def _run(x, cond, d, wt, device, **kw):
    y, s = WN.residual_layer(*_t((x, cond, d), device), wt, **kw)
    return y.cpu().numpy().astype(np.float64), s.cpu().numpy().astype(np.float64)


def _inputs(rng, B, C, T):
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    cond = rng.standard_normal((B, H, T)).astype(np.float32)
    d = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
    return x, cond, d


def _check(tag, got, ref, bars):
    """print and assert err <= bar for (x_out, skip); returns the worst err / bar"""
    worst = 0.0
    for name, g, r, bar in zip(("x_out", "skip"), got, ref, bars):
        err = float(np.abs(g - r).max())
        print("%s %s: err %.3e bar %.3e err / bar %.3f" % (tag, name, err, bar, err / bar))
        worst = max(worst, err / bar)
        assert err <= bar, (tag, name, err, bar)
    return worst


# ---- the oracle against the reference's own output ------------------------------------------------------------------------------

def test_oracle_matches_reference_fixture():
    g = np.load(GOLDEN)
    x, cond, s = g["layer_x"], g["layer_cond"], g["layer_s"]
    assert x.shape == (2, 32, 70) and cond.shape == (2, 16, 70)
    weights, proj = tuple(g["layer_" + n] for n in NAMES), (g["layer_wp"], g["layer_bp"])
    d = O.project(s, proj)
    want = O.layer(x, cond, d, weights)
    chain = _torch_stack(x, cond, s, [(weights, proj)])
    for w, c, name in zip(want, (chain[0], chain[1]), ("layer_x_out", "layer_skip")):
        assert np.abs(g[name] - w).max() <= 1e-5 * _rms(w)
        assert np.abs(c - g[name]).max() <= 1e-5 * _rms(w)
    # the 3-layer net: what its first layer received -> what skip_projection received -> the output
    layers = [(O.seeded_weights(32, 16, 10 + i), O.seeded_projection(32, 20 + i)) for i in range(3)]
    _, total = O.stack(g["net_x0"], g["net_cond"], g["net_s"], layers)
    skip_in = total / np.sqrt(3.0)
    assert np.abs(g["net_skip_in"] - skip_in).max() <= 1e-5 * _rms(skip_in)
    h = np.maximum(np.einsum("oc,bct->bot", g["net_sp_w"][:, :, 0].astype(np.float64), skip_in) + g["net_sp_b"][None, :, None], 0.0)
    y = np.einsum("oc,bct->bot", g["net_op_w"][:, :, 0].astype(np.float64), h) + g["net_op_b"][None, :, None]
    assert _rms(y) > 0.1 and np.abs(g["net_y"][:, 0] - y).max() <= 1e-5 * _rms(y)
    _, chain_total = _torch_stack(g["net_x0"], g["net_cond"], g["net_s"], layers)
    assert np.abs(chain_total / np.float32(np.sqrt(3.0)) - g["net_skip_in"]).max() <= 1e-5 * _rms(skip_in)


@pytest.mark.parametrize("C,Hc", SHAPES + ((32, 16),))
def test_seeded_weights_put_z_in_the_curved_range_and_o_at_the_size_of_x(C, Hc):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, C, 16))
    cond, s = rng.standard_normal((1, Hc, 16)), rng.standard_normal((1, C))
    weights = O.seeded_weights(C, Hc, 1)
    d = O.project(s, O.seeded_projection(C, 2))
    assert 0.7 < _rms(O.z_of(x, cond, d, weights)) < 1.4
    x_out, skip = O.layer(x, cond, d, weights)
    assert 0.5 * _rms(x) < _rms(x_out * np.sqrt(2.0) - x) < 2.0 * _rms(x)
    assert 0.5 * _rms(x) < _rms(skip) < 2.0 * _rms(x)


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("C,Hc", SHAPES)
def test_parity(dev, C, Hc):
    t = WN.tile(C, Hc)
    assert t == 64
    weights = O.seeded_weights(C, Hc, 10)
    wt = _t(weights, dev)
    rng = np.random.default_rng(C)
    worst = 0.0
    for T in (1, 2, 3, 5, t - 1, t, t + 1, 2 * t + 5):
        x, cond, d = _inputs(rng, 2, C, T)
        assert not np.array_equal(x[0], x[1])
        ref = O.layer(x, cond, d, weights)
        bars = _bars(_torch_layer(x, cond, d, weights), ref)
        worst = max(worst, _check("C %d T %d" % (C, T), _run(x, cond, d, wt, dev), ref, bars))
    print("C %d worst err / bar %.3f" % (C, worst))


# ---- edges: the convolution pads its own input ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_x_plus_d_is_zero_outside_the_sequence(dev):
    C = 384
    t = WN.tile(C, H)
    weights = O.seeded_weights(C, H, 20)
    wt = _t(weights, dev)
    rng = np.random.default_rng(21)
    for T in (1, t, t + 1):
        x = np.zeros((1, C, T), np.float32)
        cond = rng.standard_normal((1, H, T)).astype(np.float32)
        d = (10.0 * np.sign(rng.standard_normal((1, C)))).astype(np.float32)
        ref = O.layer(x, cond, d, weights)
        bars = _bars(_torch_layer(x, cond, d, weights), ref)
        got = _run(x, cond, d, wt, dev)
        wrong = O.layer(x, cond, d, weights, pad_with_d=True)
        for f in sorted({0, T - 1}):
            edge = lambda pair: tuple(a[:, :, f] for a in pair)
            _check("T %d frame %d" % (T, f), edge(got), edge(ref), bars)
            for w, r, bar in zip(edge(wrong), edge(ref), bars):
                assert np.abs(w - r).max() > 10 * bar, (T, f)                       # the case can fail
        _check("T %d" % T, got, ref, bars)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_halves_and_tap_orientation(dev):
    C, T = 384, 5
    rng = np.random.default_rng(31)
    x, cond, d = _inputs(rng, 1, C, T)
    base = O.seeded_weights(C, H, 30)

    def case(tag, weights, **variant):
        ref = O.layer(x, cond, d, weights)
        bars = _bars(_torch_layer(x, cond, d, weights), ref)
        _check(tag, _run(x, cond, d, _t(weights, dev), dev), ref, bars)
        wrong = O.layer(x, cond, d, weights, **variant)
        for w, r, bar in zip(wrong, ref, bars):
            assert np.abs(w - r).max() > 10 * bar, tag

    wdil, bdil, wc, bc, wo, bo = [a.copy() for a in base]
    bdil[:C] += 4.0                                    # gate rows large positive, filter rows small
    wdil[C:] *= 0.1
    wc[C:] *= 0.1
    case("gate / filter", (wdil, bdil, wc, bc, wo, bo), swap_gate=True)
    wdil, bdil, wc, bc, wo, bo = [a.copy() for a in base]
    wo[C:] *= 3.0                                      # the skip half three times the residual half
    case("residual / skip", (wdil, bdil, wc, bc, wo, bo), swap_out=True)
    for k in (0, 2):
        wdil = base[0].copy()
        wdil[:, :, [j for j in range(3) if j != k]] = 0.0
        case("one-hot tap %d" % k, (wdil * np.float32(1.7),) + base[1:], flip_taps=True)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_saturation(dev):
    """z = +-200 on both halves in all four sign pairs: expf overflows, the outputs are the limits (sigmoid 0 / 1, tanh +-1)"""
    C, T = 384, 3
    rng = np.random.default_rng(41)
    x, cond, d = _inputs(rng, 1, C, T)
    wdil, bdil, wc, bc, wo, bo = [a.copy() for a in O.seeded_weights(C, H, 40)]
    wdil[:], wc[:], bc[:] = 0.0, 0.0, 0.0
    c = np.arange(C)
    bdil[:C] = np.where(c & 1, 200.0, -200.0)
    bdil[C:] = np.where(c & 2, 200.0, -200.0)
    weights = (wdil, bdil, wc, bc, wo, bo)
    z = O.z_of(x, cond, d, weights)
    assert np.all(np.abs(z) == 200.0)
    g = np.where(c & 1, 1.0, 0.0) * np.where(c & 2, 1.0, -1.0)
    limit = wo[:, :, 0].astype(np.float64) @ g + bo
    ref = O.layer(x, cond, d, weights)
    assert np.abs(ref[1] - limit[None, C:, None]).max() <= 1e-12
    got = _run(x, cond, d, _t(weights, dev), dev)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    _check("saturated", got, ref, _bars(_torch_layer(x, cond, d, weights), ref))


# ---- the stack, the running skip sum and the packed cache -------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_stack_skip_accumulation_and_packed_cache(dev):
    C, B, T = 384, 2, 7
    layers = [(O.seeded_weights(C, H, 50 + i), O.seeded_projection(C, 60 + i)) for i in range(3)]
    lt = [(_t(w, dev), _t(p, dev)) for w, p in layers]
    rng = np.random.default_rng(51)
    x, cond, _ = _inputs(rng, B, C, T)
    s = rng.standard_normal((B, C)).astype(np.float32)
    xt, ct, st = _t((x, cond, s), dev)
    ref = O.stack(x, cond, s, layers)
    bars = _bars(_torch_stack(x, cond, s, layers), ref)
    p0 = WN.PACKS["count"]
    y, total = WN.residual_stack(xt, ct, st, lt)
    assert WN.PACKS["count"] == p0 + 3
    assert torch.equal(xt.cpu(), torch.from_numpy(x)) and torch.equal(ct.cpu(), torch.from_numpy(cond))   # never written
    _check("stack", (y.cpu().numpy(), total.cpu().numpy()), ref, bars)
    # a non-contiguous cond (the [B, T, H] tensor seen through transpose(1, 2)) gives the same bits
    view = ct.transpose(1, 2).contiguous().transpose(1, 2)
    assert not view.is_contiguous()
    y2, total2 = WN.residual_stack(xt, view, st, lt)
    assert torch.equal(y2, y) and torch.equal(total2, total)
    assert WN.PACKS["count"] == p0 + 3                                            # the second call found the cached tables
    # accumulate adds exactly the layer's skip to what the buffer holds
    d = torch.from_numpy(O.project(s, layers[0][1]).astype(np.float32)).to(dev)
    _, plain = WN.residual_layer(xt, ct, d, lt[0][0])
    preset = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(dev)
    buf = preset.clone()
    _, got = WN.residual_layer(xt, ct, d, lt[0][0], skip=buf, accumulate=True)
    assert got is buf and torch.equal(buf, preset + plain)
    for bad in (dict(out=xt), dict(skip=xt), dict(accumulate=True)):
        with pytest.raises(ValueError):
            WN.residual_layer(xt, ct, d, lt[0][0], **bad)
    # an in-place write bumps _version: one table is rebuilt and the result follows the new weight
    p1 = WN.PACKS["count"]
    lt[2][0][4].mul_(-1.5)
    layers[2] = (tuple(a if i != 4 else a * np.float32(-1.5) for i, a in enumerate(layers[2][0])), layers[2][1])
    y3, total3 = WN.residual_stack(xt, ct, st, lt)
    assert WN.PACKS["count"] == p1 + 1
    ref3 = O.stack(x, cond, s, layers)
    bars3 = _bars(_torch_stack(x, cond, s, layers), ref3)
    assert np.abs(ref3[1] - ref[1]).max() > 100 * bars3[1]
    _check("stack, new weight", (y3.cpu().numpy(), total3.cpu().numpy()), ref3, bars3)


# ---- batch split ------------------------------------------------------------------------------------------------------------------

def _rows_differ(a):
    a = np.asarray(a).reshape(len(a), -1)
    for i in range(a.shape[0]):
        for j in range(i + 1, a.shape[0]):
            assert not np.array_equal(a[i], a[j]), (i, j)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_batch_split(dev, knobs):
    """BATCH_SPLIT 2 and 1 at B = 5: chunks 2, 2, 1 (two non-zero bases, an uneven tail) meet two tiles"""
    C = 384
    T = WN.tile(C, H) + 1
    weights = O.seeded_weights(C, H, 70)
    wt = _t(weights, dev)
    x, cond, d = _inputs(np.random.default_rng(72), 5, C, T)
    ref = O.layer(x, cond, d, weights)
    bars = _bars(_torch_layer(x, cond, d, weights), ref)
    xt, ct, dt = _t((x, cond, d), dev)
    whole = WN.residual_layer(xt, ct, dt, wt, out=torch.full_like(xt, NAN), skip=torch.full_like(xt, NAN))
    _check("B 5", tuple(a.cpu().numpy() for a in whole), ref, bars)
    _rows_differ(ref[0])
    _rows_differ(ref[1])
    for split in (2, 1):
        knobs("BATCH_SPLIT", split)
        part = WN.residual_layer(xt, ct, dt, wt, out=torch.full_like(xt, NAN), skip=torch.full_like(xt, NAN))
        for p, w in zip(part, whole):
            assert torch.isfinite(p).all(), split
            assert torch.equal(p, w), split


@pytest.mark.gpu
def test_past_the_grid_limit():
    """B = 65 537 = 65 535 + 2 at T = 4, utterance b = pool[b % 251] (251 is prime and 65 535 mod 251 = 24: a wrong base or stride
    moves an utterance onto another pool entry), compared bitwise with the pool's own run, which the oracle checks.  403 MB per
    [B, 384, 4] tensor."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    C, POOL, B, T = 384, 251, 65535 + 2, 4
    weights = O.seeded_weights(C, H, 80)
    wt = _t(weights, device)
    xp, cp, dp = _inputs(np.random.default_rng(81), POOL, C, T)
    ref = O.layer(xp, cp, dp, weights)
    bars = _bars(_torch_layer(xp, cp, dp, weights), ref)
    xpool, cpool, dpool = _t((xp, cp, dp), device)
    ypool, spool = WN.residual_layer(xpool, cpool, dpool, wt)
    _check("pool", (ypool.cpu().numpy(), spool.cpu().numpy()), ref, bars)
    _rows_differ(ref[0])
    idx = torch.arange(B, device=device) % POOL
    x, cond, d = xpool[idx].contiguous(), cpool[idx].contiguous(), dpool[idx].contiguous()
    y, s = WN.residual_layer(x, cond, d, wt, out=torch.full_like(x, NAN), skip=torch.full_like(x, NAN))
    assert torch.isfinite(y).all() and torch.isfinite(s).all()
    assert torch.equal(y, ypool[idx]) and torch.equal(s, spool[idx])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    C = 384
    outside = ((256, 256), (384, 128), (0, 0), (-384, 256), (384, -256))
    assert [lib.ddsp_hip_wavenet_layer_tile(c, h) for c, h in SHAPES] == [64, 64]
    assert [lib.ddsp_hip_wavenet_layer_tile(c, h) for c, h in outside] == [0] * 5
    floats = lambda c, h: 2 * c * (3 * c + h) + 2 * c * c + 4 * c
    assert [lib.ddsp_hip_wavenet_layer_pack_bytes(c, h) for c, h in SHAPES] == [4 * floats(c, h) for c, h in SHAPES]
    assert [lib.ddsp_hip_wavenet_layer_pack_bytes(c, h) for c, h in outside] == [0] * 5
    weights = O.seeded_weights(C, H, 90)
    w = [torch.from_numpy(a) for a in weights]
    need = 4 * floats(C, H)
    tab = torch.zeros(need // 4)
    ptrs = [a.data_ptr() for a in w]
    pack = lambda p, c=C, h=H, n=need: lib.ddsp_hip_wavenet_layer_pack(*p, c, h, tab.data_ptr(), n)
    assert pack(ptrs, n=need - 4) == -4
    assert pack(ptrs, c=256) == -3 and pack(ptrs, h=128) == -3
    for i in range(6):
        assert pack(ptrs[:i] + [None] + ptrs[i + 1:]) == -1
    assert pack(ptrs) == 0
    T = 6
    gen = torch.Generator().manual_seed(1)
    x, cond, d = torch.randn(2, C, T, generator=gen), torch.randn(2, H, T, generator=gen), torch.randn(2, C, generator=gen)
    y, s = torch.full((2, C, T), 7.0), torch.full((2, C, T), 7.0)
    call = lambda **kw: lib.ddsp_hip_wavenet_layer(*[kw.get(n, v) for n, v in (
        ("x", x.data_ptr()), ("cond", cond.data_ptr()), ("d", d.data_ptr()), ("y", y.data_ptr()), ("s", s.data_ptr()),
        ("t", tab.data_ptr()), ("tb", need), ("B", 2), ("T", T), ("C", C), ("H", H), ("mode", 0), ("st", None))])
    for kw, code in (({"C": 256}, -3), ({"H": 128}, -3), ({"C": 0, "H": 0}, -3), ({"T": 0}, -1), ({"T": -1}, -1),
                     ({"T": 2 ** 40 + 1}, -3), ({"B": -1}, -1), ({"tb": need - 4}, -4), ({"x": None}, -1), ({"cond": None}, -1),
                     ({"d": None}, -1), ({"y": None}, -1), ({"s": None}, -1), ({"t": None}, -1), ({"y": x.data_ptr()}, -1),
                     ({"mode": 2}, -1)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all() and (s == 7.0).all(), kw                           # refused before any launch
    assert call(B=0, x=None, y=None) == 0 and (y == 7.0).all()                     # a no-op
    assert call() == 0
    ref = O.layer(x.numpy(), cond.numpy(), d.numpy(), weights)
    assert np.abs(y.numpy() - ref[0]).max() <= 1e-5 * np.abs(ref[0]).max()
    assert np.abs(s.numpy() - ref[1]).max() <= 1e-5 * np.abs(ref[1]).max()


# ---- dispatch -------------------------------------------------------------------------------------------------------------------

def _counts():
    return WN.CALLS["hip"], WN.CALLS["reference"]


def _seeded_block(C, seed):
    return S.load(S.ResidualBlock(H, C), O.seeded_weights(C, H, seed), O.seeded_projection(C, seed + 1))


def _close(got, want):
    for g, w in zip(got, want):
        assert (g - w).abs().max() <= 1e-5 * float(w.abs().max())


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_dispatch(dev):
    from ddsp_svc_amd import conformer as CF
    cf_calls = dict(CF.CALLS)
    C, T = 384, 5
    gen = torch.Generator().manual_seed(0)
    x, cond, s = torch.randn(1, C, T, generator=gen), torch.randn(1, H, T, generator=gen), torch.randn(1, C, generator=gen)
    block = _seeded_block(C, 100)
    with torch.no_grad():
        h0, r0 = _counts()
        got = block(x, cond, s)
        assert _counts() == (h0 + 1, r0)
        _close(got, block.reference_forward(x, cond, s))

        def goes_to_reference(m, *inputs):
            h0, r0 = _counts()
            got = m(*inputs)
            assert _counts() == (h0, r0 + 1)
            for g, w in zip(got, m.reference_forward(*inputs)):
                assert torch.equal(g, w)

        goes_to_reference(S.ResidualBlock(H, C, dilation=2), x, cond, s)             # dilation 2
        goes_to_reference(S.ResidualBlock(H, C, kernel=5), x, cond, s)             # kernel 5
        wn = _seeded_block(C, 102)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.nn.utils.weight_norm(wn.output_projection)
        goes_to_reference(wn, x, cond, s)                                          # a weight-normed conv
        hooked = _seeded_block(C, 104)
        hooked.dilated_conv.register_forward_hook(lambda mod, inp, out: None)
        goes_to_reference(hooked, x, cond, s)                                      # a forward hook
        goes_to_reference(_seeded_block(C, 106).half(), x.half(), cond.half(), s.half())   # float16 parameters
        small = S.ResidualBlock(H, 256)
        goes_to_reference(small, torch.randn(1, 256, T), cond, torch.randn(1, 256))    # C = 256
        with torch.autocast("cpu", dtype=torch.bfloat16):
            h0, r0 = _counts()
            block(x, cond, s)
            assert _counts() == (h0, r0 + 1)                                       # autocast on
    xg = x.clone().requires_grad_(True)                                            # a gradient is needed
    h1, r1 = _counts()
    yg, _ = block(xg, cond, s)
    assert _counts() == (h1, r1 + 1) and yg.requires_grad
    with torch.no_grad():
        block(xg, cond, s)
        assert _counts() == (h1 + 1, r1 + 1)
    assert CF.CALLS == cf_calls                        # the conformer's counters are not touched


def test_dispatch_keeps_host_tensors_on_the_reference():
    block = S.ResidualBlock(H, 384)
    x, cond, s = torch.randn(1, 384, 3), torch.randn(1, H, 3), torch.randn(1, 384)
    with torch.no_grad():
        h0, r0 = _counts()
        got = block(x, cond, s)
        assert _counts() == (h0, r0 + 1)
        for g, w in zip(got, block.reference_forward(x, cond, s)):
            assert torch.equal(g, w)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_net_dispatch(dev):
    C, T = 384, 4
    torch.manual_seed(3)
    blocks = [_seeded_block(C, 110 + 2 * i) for i in range(3)]
    net = S.WaveNet(8, 3, C, H, blocks=blocks)
    spec, step, cond = torch.randn(1, 1, 8, T), torch.tensor([12.0]), torch.randn(1, H, T)
    with torch.no_grad():
        want = net.reference_forward(spec, step, cond)
        h0, r0 = _counts()
        got = net(spec, step, cond)
        assert _counts() == (h0 + 3, r0)                                           # the stack: one launch per layer
        assert got.shape == want.shape and (got - want).abs().max() <= 1e-5 * float(want.abs().max())
        blocks[1].dilated_conv.register_forward_hook(lambda mod, inp, out: None)
        h0, r0 = _counts()
        got = net(spec, step, cond)                                                # one ineligible layer: layer by layer
        assert _counts() == (h0 + 2, r0 + 1)
        assert (got - want).abs().max() <= 1e-5 * float(want.abs().max())


# ---- the reference hook -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_reference_hook(dev):
    ref_root = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
    if not os.path.isdir(os.path.join(ref_root, "diffusion")):
        pytest.skip("reference checkout not present (only in the build container)")
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    import diffusion.wavenet as M
    block_fwd, net_fwd = M.ResidualBlock.forward, M.WaveNet.forward
    C = 384
    torch.manual_seed(9)
    net = M.WaveNet(8, 3, C, H).eval()
    for i, layer in enumerate(net.residual_layers):     # the default initialisation would leave the residual at a few per cent
        S.load(layer, O.seeded_weights(C, H, 120 + i), O.seeded_projection(C, 130 + i))
    with torch.no_grad():
        net.output_projection.weight.normal_(0.0, C ** -0.5)                       # the reference zeroes it
    gen = torch.Generator().manual_seed(7)
    spec, step, cond = torch.randn(2, 1, 8, 70, generator=gen), torch.tensor([5.0, 60.0]), torch.randn(2, H, 70, generator=gen)
    with torch.no_grad():
        want = net(spec, step, cond)
        exact = net.double()(spec.double(), step.double(), cond.double()).numpy()
        net.float().to(dev)
        try:
            assert WN.patch_reference_wavenet() is M
            patched = M.WaveNet.forward
            assert patched is not net_fwd and M.ResidualBlock.forward is not block_fwd
            WN.patch_reference_wavenet()               # idempotent
            assert M.WaveNet.forward is patched and M.WaveNet._reference_forward is net_fwd
            assert M.ResidualBlock._reference_forward is block_fwd
            h0, r0 = _counts()
            got = net(spec.to(dev), step.to(dev), cond.to(dev))
            assert _counts() == (h0 + 3, r0)
        finally:
            WN.unpatch_reference_wavenet()
        assert M.ResidualBlock.forward is block_fwd and M.WaveNet.forward is net_fwd
        assert "_reference_forward" not in M.ResidualBlock.__dict__ and "_reference_forward" not in M.WaveNet.__dict__
    e_torch = float(np.abs(want.numpy() - exact).max())
    err = float(np.abs(got.cpu().numpy() - exact).max())
    bar = 4 * e_torch + 1e-7 * _rms(exact)
    print("WaveNet through the hook: hip %.3e torch %.3e err / bar %.3f" % (err, e_torch, err / bar))
    assert _rms(exact) > 0.1 and err <= bar


# ---- the crossover table --------------------------------------------------------------------------------------------------------

def test_crossover_table_agrees_with_the_committed_measurements():
    """every single-layer case of profiles/wavenet_{throughput,latency}.json is routed to whichever side was measured faster; a C
    without committed measurements maps to None: torch at every size"""
    cases = []
    for mode in ("throughput", "latency"):
        path = os.path.join(ROOT, "profiles", "wavenet_%s.json" % mode)
        if not os.path.exists(path):
            continue
        with open(path) as f:
            doc = json.load(f)
        assert doc["H"] == H and doc["tile"] == 64
        cases += [c for c in doc["cases"] if c["case"] == "layer"]
    measured = {c["C"] for c in cases}
    for C, _ in SHAPES:
        if C not in measured:
            assert C in SHIPPED_TORCH_FASTER and SHIPPED_TORCH_FASTER[C] is None
    if cases:
        assert {c["frames"] for c in cases} == {100, 203, 48 * 172, 32 * 862, 64 * 862}
    for c in cases:
        table, C = SHIPPED_TORCH_FASTER, c["C"]
        to_torch = C in table and (table[C] is None or c["frames"] < table[C])
        assert to_torch == (c["torch_over_hip"] < 1.0), (C, c["frames"], c["torch_over_hip"], table)


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _stack_case(device, T=70):
    C = 384
    layers = [(O.seeded_weights(C, H, 140 + i), O.seeded_projection(C, 150 + i)) for i in range(3)]
    lt = [(_t(w, device), _t(p, device)) for w, p in layers]
    gen = torch.Generator().manual_seed(4)
    x, cond, s = torch.randn(2, C, T, generator=gen), torch.randn(2, H, T, generator=gen), torch.randn(2, C, generator=gen)
    return layers, lt, x.to(device), cond.to(device), s.to(device)


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical_and_allocates_only_its_buffers():
    """the stack is a chain of launches on the caller's stream: a capture of it has no parallel branches"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    layers, lt, x, cond, s = _stack_case(device)
    eager = WN.residual_stack(x, cond, s, lt)          # the warm call packs the tables and stacks the projections
    ref = O.stack(x.cpu().numpy(), cond.cpu().numpy(), s.cpu().numpy(), layers)
    bars = _bars(_torch_stack(x.cpu().numpy(), cond.cpu().numpy(), s.cpu().numpy(), layers), ref)
    _check("stack", tuple(a.cpu().numpy() for a in eager), ref, bars)
    torch.cuda.synchronize()
    p0 = WN.PACKS["count"]
    nbytes = x.numel() * 4
    assert nbytes % 512 == 0
    d_bytes = -(-(3 * s.numel() * 4) // 512) * 512
    before = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    held = WN.residual_stack(x, cond, s, lt)
    assert torch.cuda.memory_allocated(device) - before == 2 * nbytes            # the two results stay
    assert torch.cuda.max_memory_allocated(device) - before <= 3 * nbytes + 2 * d_bytes   # + one hand-over buffer and d
    assert WN.PACKS["count"] == p0
    del held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, total = WN.residual_stack(x, cond, s, lt)
    for _ in range(2):
        y.fill_(NAN)
        total.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager[0]) and torch.equal(total, eager[1])


@pytest.mark.gpu
def test_gpu_non_default_stream_is_honoured():
    """x is produced on a side stream right before the call, without any synchronisation in between: only a launch on that same
    stream is ordered behind it"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    _, lt, x, cond, s = _stack_case(device)
    d = s.clone()
    eager = WN.residual_layer(x, cond, d, lt[0][0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    big = torch.randn(4096, 4096, device=device)
    xs = torch.zeros_like(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big @ big * 1e-2                     # keeps the side stream busy while the host runs ahead
        xs.copy_(x)
        y, sk = WN.residual_layer(xs, cond, d, lt[0][0])
    side.synchronize()
    assert torch.equal(y, eager[0]) and torch.equal(sk, eager[1])
