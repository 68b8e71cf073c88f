"""The layer of the reflow / diffusion-fast denoiser (ddsp_svc_amd.naive_v2, csrc/naive_v2_layer.h): the two HIP launches on the
emulator and the GPU against the float64 oracle, the zero padding of the GLU's output, the residual, the halves of the GLU and the
tap orientation, saturation, the stack, the input strides, the batch split, the C ABI, the dispatch and the reference hook.

The parity bar is test_conformer.py's, relative to what float32 itself does on the same inputs: with e_torch = max|the torch op
chain in float32 on the CPU - oracle|, the kernels must stay within 4 e_torch + 1e-7 rms(oracle) (another summation order over
Hc + D, 31 and 2 D terms).  Every case prints its err / bar."""
import functools
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import naive_v2_oracle as O
from tests import naive_v2_standin as S
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import _ffi, naive_v2 as NV  # noqa: E402

D, HC = 512, 128
TA, TB = 64, 112
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "naive_v2_layer.npz")
NAMES = ("wc", "bc", "w1", "b1", "wd", "bd", "w2", "b2")
NAN = float("nan")

SHIPPED_TORCH_FASTER = dict(NV.LAYER_TORCH_FASTER)


@pytest.fixture(autouse=True)
def _structural_dispatch(monkeypatch):
    """the dispatch tests decide from a module's structure at shapes of a few frames: the measured crossover table (whose own
    test reads SHIPPED_TORCH_FASTER) is empty while they run, as it is in tools/naive_v2_bench.py"""
    monkeypatch.setattr(NV, "LAYER_TORCH_FASTER", {})


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


@functools.lru_cache(maxsize=None)
def _weights(seed, d=D, hc=HC):
    return O.seeded_weights(d, hc, seed)


def _torch_layer(x, cond, d, weights):
    """the layer's op chain as torch ops in float32 on the CPU, [B, L, D] in and out"""
    x, cond, d = [torch.as_tensor(np.asarray(a, np.float32)) for a in (x, cond, d)]
    wc, bc, w1, b1, wd, bd, w2, b2 = [torch.as_tensor(a) for a in weights]
    xt = x.transpose(1, 2)
    xp = xt + d.unsqueeze(-1) + F.conv1d(cond.transpose(1, 2), wc, bc)
    g = F.glu(F.conv1d(xp, w1, b1), dim=1)
    h = F.silu(F.conv1d(g, wd, bd, padding=O.PAD, groups=wd.shape[0]))
    return (xt + F.conv1d(h, w2, b2)).transpose(1, 2).contiguous().numpy()


def _torch_stack(x, cond, s, layers):
    x, s32 = np.asarray(x, np.float32), torch.as_tensor(np.asarray(s, np.float32))
    for weights, (wp, bp) in layers:
        d = F.linear(s32, torch.as_tensor(wp)[:, :, 0], torch.as_tensor(bp)).numpy()
        x = _torch_layer(x, cond, d, weights)
    return x


def _bar(chain, ref):
    return 4.0 * float(np.abs(chain.astype(np.float64) - ref).max()) + 1e-7 * _rms(ref)


def _t(arrays, device):
    """tensors of their own: an in-place write to one must not reach the numpy arrays the oracle reads"""
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).clone().to(device) for a in arrays)


def _run(x, cond, d, wt, device, **kw):
    return NV.diff_layer(*_t((x, cond, d), device), wt, **kw).cpu().numpy().astype(np.float64)


def _inputs(rng, B, L, d=D, hc=HC):
    x = rng.standard_normal((B, L, d)).astype(np.float32)
    cond = rng.standard_normal((B, L, hc)).astype(np.float32)
    dd = (0.5 * rng.standard_normal((B, d))).astype(np.float32)
    return x, cond, dd


def _check(tag, got, ref, bar):
    err = float(np.abs(got - ref).max())
    print("%s: err %.3e bar %.3e err / bar %.3f" % (tag, err, bar, err / bar))
    assert err <= bar, (tag, err, bar)
    return err / bar


# ---- the oracle against the reference's own output ------------------------------------------------------------------------------

def test_oracle_and_torch_chain_match_the_reference_fixture():
    g = np.load(GOLDEN)
    tr = lambda a: np.ascontiguousarray(np.swapaxes(a, 1, 2))
    x, cond, s = tr(g["layer_x"]), tr(g["layer_cond"]), g["layer_step"][:, :, 0]
    assert x.shape == (2, 70, 32) and cond.shape == (2, 70, 8)
    weights, proj = tuple(g["layer_" + n] for n in NAMES), (g["layer_wp"], g["layer_bp"])
    want = O.layer(x, cond, O.project(s, proj), weights)
    have = tr(g["layer_y"])
    assert np.abs(have - want).max() <= 1e-5 * _rms(want)
    assert np.abs(_torch_stack(x, cond, s, [(weights, proj)]) - have).max() <= 1e-5 * _rms(want)
    assert 0.5 * _rms(x) < _rms(want - x) < 2.0 * _rms(x)
    # the 3-layer net: what its first layer received -> what output_projection received -> the output
    layers = [(_weights(10 + i, 32, 8), O.seeded_projection(32, 20 + i)) for i in range(3)]
    x0, cond, s = tr(g["net_x0"]), tr(g["net_cond"]), g["net_s"][:, :, 0]
    out_in = O.stack(x0, cond, s, layers)
    assert np.abs(tr(g["net_out_in"]) - out_in).max() <= 1e-5 * _rms(out_in)
    assert np.abs(_torch_stack(x0, cond, s, layers) - tr(g["net_out_in"])).max() <= 1e-5 * _rms(out_in)
    y = out_in @ g["net_op_w"][:, :, 0].astype(np.float64).T + g["net_op_b"]
    assert _rms(y) > 0.1 and np.abs(tr(g["net_y"][:, 0]) - y).max() <= 1e-5 * _rms(y)


@pytest.mark.parametrize("d,hc", ((D, HC), (32, 8)))
def test_seeded_weights_put_the_gate_in_the_curved_range_and_the_branch_at_the_size_of_x(d, hc):
    rng = np.random.default_rng(0)
    x, cond, _ = _inputs(rng, 1, 64, d, hc)
    weights = _weights(1, d, hc)
    dd = O.project(rng.standard_normal((1, d)), O.seeded_projection(d, 2))
    z = O.pre_glu(x, cond, dd, weights)
    assert 0.7 < _rms(z[..., 2 * d:]) < 1.4 and 0.7 < _rms(z[..., :2 * d]) < 1.4
    y = O.layer(x, cond, dd, weights)
    assert 0.5 * _rms(x) < _rms(y - x) < 2.0 * _rms(x)


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("L", (1, 15, 16, 31, TA - 1, TA, TA + 1, TB - 1, TB, TB + 1, 2 * max(TA, TB) + 5))
def test_parity(dev, L):
    assert NV.tile(D, HC) == (TA, TB)
    weights = _weights(10)
    x, cond, d = _inputs(np.random.default_rng(L), 2, L)
    assert not np.array_equal(x[0], x[1])
    ref = O.layer(x, cond, d, weights)
    _check("L %d" % L, _run(x, cond, d, _t(weights, dev), dev), ref, _bar(_torch_layer(x, cond, d, weights), ref))


# ---- edges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_g_is_zero_outside_the_sequence(dev):
    """d and bc of size 10: glu(W1 (d + bc) + b1) in the stencil's padding would be off by orders of magnitude"""
    L = TB + 3
    rng = np.random.default_rng(21)
    weights = list(_weights(20))
    weights[1] = (10.0 * np.sign(rng.standard_normal(D))).astype(np.float32)
    weights = tuple(weights)
    x, cond, _ = _inputs(rng, 2, L)
    d = (10.0 * np.sign(rng.standard_normal((2, D)))).astype(np.float32)
    ref = O.layer(x, cond, d, weights)
    bar = _bar(_torch_layer(x, cond, d, weights), ref)
    got = _run(x, cond, d, _t(weights, dev), dev)
    wrong = O.layer(x, cond, d, weights, leak_pad=True)
    for name, sl in (("first 15", slice(0, 15)), ("last 15", slice(L - 15, L))):
        _check("L %d %s frames" % (L, name), got[:, sl], ref[:, sl], bar)
        assert np.abs(wrong[:, sl] - ref[:, sl]).max() > 100 * bar, name           # the case can fail
    _check("L %d" % L, got, ref, bar)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_the_residual_is_x_not_x_prime(dev):
    L = 5
    rng = np.random.default_rng(25)
    weights = _weights(24)
    x, cond, _ = _inputs(rng, 2, L)
    d = (10.0 * np.sign(rng.standard_normal((2, D)))).astype(np.float32)
    ref = O.layer(x, cond, d, weights)
    bar = _bar(_torch_layer(x, cond, d, weights), ref)
    assert np.abs(O.layer(x, cond, d, weights, residual_xp=True) - ref).max() > 5.0 > 1000 * bar
    _check("residual", _run(x, cond, d, _t(weights, dev), dev), ref, bar)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_halves_and_tap_orientation(dev):
    L = 40
    rng = np.random.default_rng(31)
    x, cond, d = _inputs(rng, 2, L)
    base = _weights(30)

    def case(tag, weights, **variant):
        ref = O.layer(x, cond, d, weights)
        bar = _bar(_torch_layer(x, cond, d, weights), ref)
        _check(tag, _run(x, cond, d, _t(weights, dev), dev), ref, bar)
        assert np.abs(O.layer(x, cond, d, weights, **variant) - ref).max() > 100 * bar, tag

    w = [a.copy() for a in base]
    w[3][:2 * D] = -np.abs(w[3][:2 * D]) - 2.0         # the "out" rows sit below zero, the gate rows above: the sign tells them apart
    w[3][2 * D:] = np.abs(w[3][2 * D:]) + 2.0
    case("out / gate", tuple(w), swap_glu=True)
    # an impulse: g is non-zero in ONE inner channel (every other row of W1 and b1 is zero), and its taps are one-hot at an end
    for k, c in ((0, 5), (TAPS_LAST, 2 * D - 3)):
        w = [a.copy() for a in base]
        keep = np.zeros(4 * D, bool)
        keep[[c, 2 * D + c]] = True
        w[2][~keep] = 0.0
        w[3][~keep] = 0.0
        w[4][:] = 0.0
        w[4][c, 0, k] = 3.0
        case("one-hot tap %d in channel %d" % (k, c), tuple(w), flip_taps=True)


TAPS_LAST = O.TAPS - 1


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_saturation(dev):
    """gate pre-activations of +-100 (expf overflows: the sigmoid is 0 or 1), then stencil outputs of +-100 (the SiLU is 100 or
    -0): finite and within the bar"""
    L = 3
    rng = np.random.default_rng(41)
    x, cond, d = _inputs(rng, 2, L)
    c = np.arange(2 * D)
    w = [a.copy() for a in _weights(40)]
    w[2][2 * D:] = 0.0
    w[3][2 * D:] = np.where(c & 1, 100.0, -100.0)
    gates = tuple(w)
    assert np.all(np.abs(O.pre_glu(x, cond, d, gates)[..., 2 * D:]) == 100.0)
    w = [a.copy() for a in _weights(40)]
    w[4][:] = 0.0
    w[5][:] = np.where(c & 2, 100.0, -100.0)
    stencils = tuple(w)
    h = np.where(c & 2, 100.0, 0.0)
    limit = stencils[6][:, :, 0].astype(np.float64) @ h + stencils[7]
    assert np.abs(O.layer(x, cond, d, stencils) - x - limit).max() <= 1e-9
    for tag, weights in (("gate +-100", gates), ("stencil +-100", stencils)):
        ref = O.layer(x, cond, d, weights)
        got = _run(x, cond, d, _t(weights, dev), dev)
        assert np.isfinite(got).all()
        _check(tag, got, ref, _bar(_torch_layer(x, cond, d, weights), ref))


# ---- the stack and the packed cache -----------------------------------------------------------------------------------------------

def _layers(seed, n):
    return [(_weights(seed + i), O.seeded_projection(D, seed + 10 + i)) for i in range(n)]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_stack_and_packed_cache(dev):
    B, L = 2, 7
    layers = _layers(50, 3)
    lt = [(_t(w, dev), _t(p, dev)) for w, p in layers]
    rng = np.random.default_rng(51)
    x, cond, _ = _inputs(rng, B, L)
    s = rng.standard_normal((B, D)).astype(np.float32)
    xt, ct, st = _t((x, cond, s), dev)
    ref = O.stack(x, cond, s, layers)
    bar = _bar(_torch_stack(x, cond, s, layers), ref)
    p0 = NV.PACKS["count"]
    y = NV.diff_stack(xt, ct, st, lt)
    assert NV.PACKS["count"] == p0 + 3
    assert torch.equal(xt.cpu(), torch.from_numpy(x)) and torch.equal(ct.cpu(), torch.from_numpy(cond))   # never written
    _check("stack", y.cpu().numpy(), ref, bar)
    y2 = NV.diff_stack(xt, ct, st, lt)
    assert torch.equal(y2, y) and NV.PACKS["count"] == p0 + 3                      # the second call found the cached tables
    d = torch.from_numpy(O.project(s, layers[2][1]).astype(np.float32)).to(dev)
    for bad in (dict(out=xt), dict(out=torch.empty(B, L, D + 1, device=dev)), dict(out=torch.empty(B, L, D, dtype=torch.float64, device=dev))):
        with pytest.raises(ValueError):
            NV.diff_layer(xt, ct, d, lt[2][0], **bad)
    with pytest.raises(ValueError):
        NV.diff_layer(xt, ct[:, :, :64], d, lt[2][0])
    with pytest.raises(ValueError):
        NV.diff_layer(xt, ct, d, lt[2][0][:6])
    for bad in ((xt, ct, st[:, :D - 1], lt), (xt, ct, st.double(), lt), (xt[0], ct, st, lt), (xt, ct, st, [])):
        with pytest.raises(ValueError):
            NV.diff_stack(*bad)
    assert NV.PACKS["count"] == p0 + 3
    # an in-place write bumps _version: that table is rebuilt and the result follows the new weight
    lt[2][0][6].mul_(-1.5)
    changed = tuple(a if i != 6 else a * np.float32(-1.5) for i, a in enumerate(layers[2][0]))
    y3 = NV.diff_layer(xt, ct, d, lt[2][0])
    assert NV.PACKS["count"] == p0 + 4
    ref3 = O.layer(x, cond, d.cpu().numpy(), changed)
    bar3 = _bar(_torch_layer(x, cond, d.cpu().numpy(), changed), ref3)
    assert np.abs(ref3 - O.layer(x, cond, d.cpu().numpy(), layers[2][0])).max() > 100 * bar3
    _check("new weight", y3.cpu().numpy(), ref3, bar3)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_input_strides(dev):
    """the reference's [B, D, L] contiguous and a transposed view of a contiguous [B, L, D] give the same bits"""
    L = 5
    layer = O.load(S.DiffLayer(D, HC), _weights(60), O.seeded_projection(D, 61)).to(dev)
    gen = torch.Generator().manual_seed(6)
    x, cond, step = torch.randn(2, D, L, generator=gen), torch.randn(2, HC, L, generator=gen), torch.randn(2, D, 1, generator=gen)
    x, cond, step = x.to(dev), cond.to(dev), step.to(dev)
    views = x.transpose(1, 2).contiguous().transpose(1, 2), cond.transpose(1, 2).contiguous().transpose(1, 2)
    assert x.is_contiguous() and not views[0].is_contiguous() and torch.equal(views[0], x)
    with torch.no_grad():
        h0 = NV.CALLS["hip"]
        a = layer(x, cond, step)
        b = layer(views[0], views[1], step)
        assert NV.CALLS["hip"] == h0 + 2
        want = layer.reference_forward(x, cond, step)
    assert a.shape == want.shape == (2, D, L) and a.stride() == b.stride() == (L * D, 1, D)    # a view of the [B, L, D] result
    assert torch.equal(a, b)
    assert (a - want).abs().max() <= 1e-5 * float(want.abs().max())


# ---- batch split ------------------------------------------------------------------------------------------------------------------

def _rows_differ(a):
    a = np.asarray(a).reshape(len(a), -1)
    for i in range(a.shape[0]):
        for j in range(i + 1, a.shape[0]):
            assert not np.array_equal(a[i], a[j]), (i, j)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_batch_split(dev, knobs):
    """BATCH_SPLIT 2 and 1 at B = 5: chunks 2, 2, 1 (two non-zero bases for x, cond, d, the workspace and y; an uneven tail)"""
    L = TA + 1
    weights = _weights(70)
    wt = _t(weights, dev)
    x, cond, d = _inputs(np.random.default_rng(72), 5, L)
    ref = O.layer(x, cond, d, weights)
    bar = _bar(_torch_layer(x, cond, d, weights), ref)
    xt, ct, dt = _t((x, cond, d), dev)
    whole = NV.diff_layer(xt, ct, dt, wt, out=torch.full_like(xt, NAN))
    _check("B 5", whole.cpu().numpy(), ref, bar)
    _rows_differ(ref)
    for split in (2, 1):
        knobs("BATCH_SPLIT", split)
        part = NV.diff_layer(xt, ct, dt, wt, out=torch.full_like(xt, NAN))
        assert torch.isfinite(part).all(), split
        assert torch.equal(part, whole), split


@pytest.mark.gpu
def test_past_the_grid_limit():
    """B = 65 537 = 65 535 + 2 at L = 2, utterance b = pool[b % 251] (251 is prime and 65 535 mod 251 = 24: a wrong base or stride
    moves an utterance onto another pool entry), compared bitwise with the pool's own run, which the oracle checks.  268 MB per
    [B, 2, 512] tensor, 537 MB of workspace."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    POOL, B, L = 251, 65535 + 2, 2
    weights = _weights(80)
    wt = _t(weights, device)
    xp, cp, dp = _inputs(np.random.default_rng(81), POOL, L)
    ref = O.layer(xp, cp, dp, weights)
    bar = _bar(_torch_layer(xp, cp, dp, weights), ref)
    xpool, cpool, dpool = _t((xp, cp, dp), device)
    ypool = NV.diff_layer(xpool, cpool, dpool, wt)
    _check("pool", ypool.cpu().numpy(), ref, bar)
    _rows_differ(ref)
    idx = torch.arange(B, device=device) % POOL
    x, cond, d = xpool[idx].contiguous(), cpool[idx].contiguous(), dpool[idx].contiguous()
    y = NV.diff_layer(x, cond, d, wt, out=torch.full_like(x, NAN))
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx])
    NV.release_workspace()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    outside = ((256, 128), (512, 256), (0, 0), (-512, 128), (512, -128))
    assert [lib.ddsp_hip_naive_v2_layer_tile(D, HC, w) for w in (0, 1, 2, -1)] == [TA, TB, 0, 0]
    assert [lib.ddsp_hip_naive_v2_layer_tile(d, h, w) for d, h in outside for w in (0, 1)] == [0] * 10
    floats = D * HC + D + 4 * D * D + 4 * D + 2 * D * 31 + 2 * D + D * 2 * D + D
    assert lib.ddsp_hip_naive_v2_layer_pack_bytes(D, HC) == 4 * floats
    assert [lib.ddsp_hip_naive_v2_layer_pack_bytes(d, h) for d, h in outside] == [0] * 5
    ws_bytes = lib.ddsp_hip_naive_v2_layer_workspace_bytes
    assert ws_bytes(2, 6, D) == 2 * 6 * 2 * D * 4 and ws_bytes(0, 6, D) == 0
    assert [ws_bytes(*a) for a in ((-1, 6, D), (2, 0, D), (2, 2 ** 30 + 1, D), (2, 6, 256))] == [0] * 4
    weights = _weights(90)
    w = [torch.from_numpy(a) for a in weights]
    need = 4 * floats
    tab = torch.zeros(need // 4)
    ptrs = [a.data_ptr() for a in w]
    pack = lambda p, d=D, h=HC, n=need: lib.ddsp_hip_naive_v2_layer_pack(*p, d, h, tab.data_ptr(), n)
    assert pack(ptrs, n=need - 4) == -4
    assert pack(ptrs, d=256) == -3 and pack(ptrs, h=256) == -3
    for i in range(8):
        assert pack(ptrs[:i] + [None] + ptrs[i + 1:]) == -1
    assert lib.ddsp_hip_naive_v2_layer_pack(*ptrs, D, HC, None, need) == -1
    assert pack(ptrs) == 0
    L = 6
    gen = torch.Generator().manual_seed(1)
    x, cond, d = torch.randn(2, L, D, generator=gen), torch.randn(2, L, HC, generator=gen), torch.randn(2, D, generator=gen)
    y = torch.full((2, L, D), 7.0)
    wsn = ws_bytes(2, L, D)
    ws = torch.zeros(wsn // 4)
    call = lambda **kw: lib.ddsp_hip_naive_v2_layer(*[kw.get(n, v) for n, v in (
        ("x", x.data_ptr()), ("cond", cond.data_ptr()), ("d", d.data_ptr()), ("y", y.data_ptr()), ("t", tab.data_ptr()), ("tb", need),
        ("ws", ws.data_ptr()), ("wb", wsn), ("B", 2), ("L", L), ("D", D), ("H", HC), ("st", None))])
    for kw, code in (({"D": 256}, -3), ({"H": 256}, -3), ({"D": 0, "H": 0}, -3), ({"L": 0}, -1), ({"L": -1}, -1),
                     ({"L": 2 ** 30 + 1}, -3), ({"B": -1}, -1), ({"tb": need - 4}, -4), ({"wb": wsn - 4}, -4), ({"x": None}, -1),
                     ({"cond": None}, -1), ({"d": None}, -1), ({"y": None}, -1), ({"t": None}, -1), ({"ws": None}, -1),
                     ({"y": x.data_ptr()}, -1), ({"y": cond.data_ptr()}, -1)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all() and (ws == 0.0).all(), kw                          # refused before any launch
    assert call(B=0, x=None, y=None, ws=None, wb=0) == 0 and (y == 7.0).all()      # a no-op
    assert call() == 0
    ref = O.layer(x.numpy(), cond.numpy(), d.numpy(), weights)
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


# ---- dispatch -------------------------------------------------------------------------------------------------------------------

def _counts():
    return NV.CALLS["hip"], NV.CALLS["reference"]


def _seeded_layer(seed, d=D, hc=HC, **kw):
    return O.load(S.DiffLayer(d, hc, **kw), O.seeded_weights(d, hc, seed), O.seeded_projection(d, seed + 1)).eval()


def _goes_to_reference(m, *inputs):
    h0, r0 = _counts()
    torch.manual_seed(5)
    got = m(*inputs)
    assert _counts() == (h0, r0 + 1)
    torch.manual_seed(5)
    want = m.reference_forward(*inputs)
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_dispatch(dev):
    from ddsp_svc_amd import conformer as CF
    cf_calls = dict(CF.CALLS)
    L = 5
    gen = torch.Generator().manual_seed(0)
    x, cond, step = torch.randn(1, D, L, generator=gen), torch.randn(1, HC, L, generator=gen), torch.randn(1, D, 1, generator=gen)
    layer = _seeded_layer(100)
    with torch.no_grad():
        h0, r0 = _counts()
        got = layer(x, cond, step)
        assert _counts() == (h0 + 1, r0)
        want = layer.reference_forward(x, cond, step)
        assert (got - want).abs().max() <= 1e-5 * float(want.abs().max())
        _goes_to_reference(_seeded_layer(102, attn=S.ScaleAttn()), x, cond, step)   # the attention half
        _goes_to_reference(_seeded_layer(104, wavenet_like=True), x, cond, step)    # wavenet_like: returns a pair
        _goes_to_reference(_seeded_layer(106, use_norm=True), x, cond, step)        # LayerNorm in the conv module
        _goes_to_reference(_seeded_layer(108, dropout=0.5).train(), x, cond, step)  # an active dropout
        _goes_to_reference(_seeded_layer(110).double(), x.double(), cond.double(), step.double())   # float64
        hooked = _seeded_layer(112)
        hooked.condition_projection.register_forward_hook(lambda mod, inp, out: None)
        _goes_to_reference(hooked, x, cond, step)                                  # a forward hook
        _goes_to_reference(_seeded_layer(114, 256), torch.randn(1, 256, L), cond, torch.randn(1, 256, 1))   # D = 256
        _goes_to_reference(_seeded_layer(116, D, 256), x, torch.randn(1, 256, L), step)                 # Hc = 256
        with torch.autocast("cpu", dtype=torch.bfloat16):
            h0, r0 = _counts()
            layer(x, cond, step)
            assert _counts() == (h0, r0 + 1)                                       # autocast on
    xg = x.clone().requires_grad_(True)                                            # a gradient is needed
    h1, r1 = _counts()
    yg = layer(xg, cond, step)
    assert _counts() == (h1, r1 + 1) and yg.requires_grad
    with torch.no_grad():
        layer(xg, cond, step)
        assert _counts() == (h1 + 1, r1 + 1)
    assert CF.CALLS == cf_calls                        # the conformer's counters are not touched


def test_dispatch_keeps_host_tensors_on_the_reference():
    layer = S.DiffLayer(D, HC).eval()
    with torch.no_grad():
        _goes_to_reference(layer, torch.randn(1, D, 3), torch.randn(1, HC, 3), torch.randn(1, D, 1))


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_net_dispatch(dev, monkeypatch):
    L = 4
    torch.manual_seed(3)
    layers = [_seeded_layer(120 + 2 * i) for i in range(2)]
    net = S.Diff(8, D, HC, layers=layers).eval()
    spec, step, cond = torch.randn(1, 1, 8, L), torch.tensor([12.0]), torch.randn(1, HC, L)
    close = lambda got, want: got.shape == want.shape and (got - want).abs().max() <= 1e-5 * float(want.abs().max())
    stacks, stack = [], NV.diff_stack
    monkeypatch.setattr(NV, "diff_stack", lambda *a: stacks.append(len(a[3])) or stack(*a))
    with torch.no_grad():
        want = net.plain_forward(spec, step, cond)                                 # no dispatcher anywhere
        assert want.dim() == 4
        h0, r0 = _counts()
        got = net(spec, step, cond)
        assert _counts() == (h0 + 2, r0) and stacks == [2]                         # the stack: one launch pair per layer
        assert close(got, want)
        assert close(net(spec[:, 0], step, cond), want[:, 0]) and stacks == [2, 2]     # 3-dim in, 3-dim out
        net.mask_cond_ratio = 0.5                                                  # the module's own forward, layer by layer
        h0, r0 = _counts()
        got = net(spec, step, cond)
        assert _counts() == (h0 + 2, r0) and len(stacks) == 2
        assert close(got, want)
        net.mask_cond_ratio = None
        layers[1].condition_projection.register_forward_hook(lambda mod, inp, out: None)
        h0, r0 = _counts()
        got = net(spec, step, cond)                                                # one ineligible layer: layer by layer
        assert _counts() == (h0 + 1, r0 + 1) and len(stacks) == 2
        assert close(got, want)
    h0, r0 = _counts()
    layers[1].condition_projection._forward_hooks.clear()
    got = net(spec, step, cond)                                                    # parameters that need a gradient: nothing computed twice
    assert _counts() == (h0, r0 + 2) and len(stacks) == 2 and got.requires_grad


# ---- the reference hook -----------------------------------------------------------------------------------------------------------

def _standin_module(name):
    """a module object with the two class names, whose forwards are the reference's own op chain"""
    mod = types.ModuleType(name)

    class NaiveV2DiffLayer(S.DiffLayer):
        forward = S.DiffLayer.reference_forward

    class NaiveV2Diff(S.Diff):
        forward = S.Diff.reference_forward             # every layer through its own forward

    mod.NaiveV2DiffLayer, mod.NaiveV2Diff = NaiveV2DiffLayer, NaiveV2Diff
    return mod


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_hook_round_trip_on_standin_modules(dev, monkeypatch):
    M = _standin_module("reflow.naive_v2_diff")
    monkeypatch.setitem(sys.modules, "reflow.naive_v2_diff", M)
    layer_fwd, net_fwd = M.NaiveV2DiffLayer.forward, M.NaiveV2Diff.forward
    torch.manual_seed(8)
    layers = [O.load(M.NaiveV2DiffLayer(D, HC), _weights(130 + i), O.seeded_projection(D, 140 + i)) for i in range(2)]
    net = M.NaiveV2Diff(8, D, HC, layers=layers).eval()
    spec, step, cond = torch.randn(1, 1, 8, 4), torch.tensor([7.0]), torch.randn(1, HC, 4)
    with torch.no_grad():
        h0, r0 = _counts()
        want = net(spec, step, cond)
        assert _counts() == (h0, r0)
        try:
            assert M in NV.patch_reference_naive_v2()
            patched = M.NaiveV2Diff.forward
            assert patched is not net_fwd and M.NaiveV2DiffLayer.forward is not layer_fwd
            NV.patch_reference_naive_v2()              # idempotent
            assert M.NaiveV2Diff.forward is patched and M.NaiveV2Diff._reference_forward is net_fwd
            assert M.NaiveV2DiffLayer._reference_forward is layer_fwd
            got = net(spec, step, cond)
            assert _counts() == (h0 + 2, r0)
            one = M.NaiveV2DiffLayer(D, HC).double()(torch.randn(1, D, 4).double(), cond.double(), torch.randn(1, D, 1).double())   # the parked forward
            assert _counts() == (h0 + 2, r0 + 1) and one.dtype == torch.float64
        finally:
            NV.unpatch_reference_naive_v2()
        assert M.NaiveV2DiffLayer.forward is layer_fwd and M.NaiveV2Diff.forward is net_fwd
        assert "_reference_forward" not in M.NaiveV2DiffLayer.__dict__ and "_reference_forward" not in M.NaiveV2Diff.__dict__
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_reference_hook(dev):
    ref_root = os.environ.get("DDSP_REFERENCE_PATH", os.path.join(os.path.dirname(ROOT), "reference"))
    if not os.path.isdir(os.path.join(ref_root, "reflow")):
        pytest.skip("reference checkout not present (set DDSP_REFERENCE_PATH, or put it beside the repository)")
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    import reflow.naive_v2_diff as M
    layer_fwd, net_fwd = M.NaiveV2DiffLayer.forward, M.NaiveV2Diff.forward
    torch.manual_seed(9)
    net = M.NaiveV2Diff(mel_channels=8, dim=D, use_mlp=False, condition_dim=HC, num_layers=2).eval()
    for i, layer in enumerate(net.residual_layers):     # the default initialisation would leave the branch at a few per cent
        O.load(layer, _weights(150 + i), O.seeded_projection(D, 160 + i))
    with torch.no_grad():
        net.output_projection.weight.normal_(0.0, D ** -0.5)                       # the reference zeroes it
    gen = torch.Generator().manual_seed(7)
    spec, step, cond = torch.randn(2, 1, 8, 40, generator=gen), torch.tensor([5.0, 60.0]), torch.randn(2, HC, 40, generator=gen)
    with torch.no_grad():
        want = net(spec, step, cond)
        exact = net.double()(spec.double(), step.double(), cond.double()).numpy()
        net.float().to(dev)
        try:
            assert M in NV.patch_reference_naive_v2()
            assert M.NaiveV2Diff._reference_forward is net_fwd and M.NaiveV2DiffLayer._reference_forward is layer_fwd
            h0, r0 = _counts()
            got = net(spec.to(dev), step.to(dev), cond.to(dev))
            assert _counts() == (h0 + 2, r0)
        finally:
            NV.unpatch_reference_naive_v2()
        assert M.NaiveV2DiffLayer.forward is layer_fwd and M.NaiveV2Diff.forward is net_fwd
    e_torch = float(np.abs(want.numpy() - exact).max())
    err = float(np.abs(got.cpu().numpy() - exact).max())
    bar = 4 * e_torch + 1e-7 * _rms(exact)
    print("NaiveV2Diff through the hook: hip %.3e torch %.3e err / bar %.3f" % (err, e_torch, err / bar))
    assert got.shape == want.shape and _rms(exact) > 0.1 and err <= bar


# ---- the crossover table --------------------------------------------------------------------------------------------------------

def test_crossover_table_agrees_with_the_committed_measurements():
    """every single-layer case of profiles/naive_v2_{throughput,latency}.json is routed to whichever side was measured faster; a D
    without committed measurements maps to None: torch at every size"""
    cases = []
    for mode in ("throughput", "latency"):
        path = os.path.join(ROOT, "profiles", "naive_v2_%s.json" % mode)
        if not os.path.exists(path):
            continue
        with open(path) as f:
            doc = json.load(f)
        assert doc["Hc"] == HC and doc["tile"] == [TA, TB]
        cases += [c for c in doc["cases"] if c["case"] == "layer"]
    measured = {c["D"] for c in cases}
    for d, _ in NV.SHAPES:
        if d not in measured:
            assert d in SHIPPED_TORCH_FASTER and SHIPPED_TORCH_FASTER[d] is None
    if cases:
        assert {c["frames"] for c in cases} == {100, 203, 48 * 172, 32 * 862, 64 * 862}
    for c in cases:
        table, d = SHIPPED_TORCH_FASTER, c["D"]
        to_torch = d in table and (table[d] is None or c["frames"] < table[d])
        assert to_torch == (c["torch_over_hip"] < 1.0), (d, c["frames"], c["torch_over_hip"], table)


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _stack_case(device, L=70):
    layers = _layers(170, 3)
    lt = [(_t(w, device), _t(p, device)) for w, p in layers]
    gen = torch.Generator().manual_seed(4)
    x, cond, s = torch.randn(2, L, D, generator=gen), torch.randn(2, L, HC, generator=gen), torch.randn(2, D, generator=gen)
    return layers, lt, x.to(device), cond.to(device), s.to(device)


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical_and_allocates_only_its_buffers():
    """the stack is a chain of launches on the caller's stream: a capture of it has no parallel branches"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    layers, lt, x, cond, s = _stack_case(device)
    eager = NV.diff_stack(x, cond, s, lt)              # the warm call packs the tables, stacks the projections, sizes the workspace
    ref = O.stack(x.cpu().numpy(), cond.cpu().numpy(), s.cpu().numpy(), layers)
    _check("stack", eager.cpu().numpy(), ref, _bar(_torch_stack(x.cpu().numpy(), cond.cpu().numpy(), s.cpu().numpy(), layers), ref))
    torch.cuda.synchronize()
    p0 = NV.PACKS["count"]
    nbytes = x.numel() * 4
    assert nbytes % 512 == 0
    d_bytes = -(-(3 * s.numel() * 4) // 512) * 512
    before = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    held = NV.diff_stack(x, cond, s, lt)
    assert torch.cuda.memory_allocated(device) - before == nbytes                # the result stays
    assert torch.cuda.max_memory_allocated(device) - before <= 2 * nbytes + 2 * d_bytes   # + one hand-over buffer and d
    assert NV.PACKS["count"] == p0
    del held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = NV.diff_stack(x, cond, s, lt)
    for _ in range(2):
        y.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)


@pytest.mark.gpu
def test_gpu_non_default_stream_is_honoured():
    """x is produced on a side stream right before the call, without any synchronisation in between: only launches on that same
    stream are ordered behind it"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    _, lt, x, cond, s = _stack_case(device)
    d = s.clone()
    eager = NV.diff_layer(x, cond, d, lt[0][0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    big = torch.randn(4096, 4096, device=device)
    xs = torch.zeros_like(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big @ big * 1e-2                     # keeps the side stream busy while the host runs ahead
        xs.copy_(x)
        y = NV.diff_layer(xs, cond, d, lt[0][0])
    side.synchronize()
    assert torch.equal(y, eager)
