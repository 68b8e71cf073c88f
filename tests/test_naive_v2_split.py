"""The channel-split form of the reflow / diffusion-fast denoiser's layer (ddsp_svc_amd.naive_v2 with form="split",
csrc/naive_v2_split.h): four launches with a frame tile of 16, on the emulator and the GPU against the float64 oracle and, bit for
bit, against the tiled form (csrc/naive_v2_layer.h), whose sums it repeats in the same order; the stack, the range, the C ABI, the
three-way dispatch (split form, tiled form, torch) and the committed crossover table.

The parity bar is test_naive_v2.py's: 4 e_torch + 1e-7 rms(oracle), e_torch the error of the float32 torch op chain on the CPU on
the same inputs.  Every case prints its err / bar."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import naive_v2_oracle as O
from tests import naive_v2_standin as S
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_naive_v2 import (_bar, _check, _inputs, _layers, _rows_differ, _standin_module, _t, _torch_layer, _torch_stack,
                                 _weights)

from ddsp_svc_amd import _ffi, naive_v2 as NV  # noqa: E402

D, HC = 512, 128
T = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "naive_v2_split_latency.json")
NAN = float("nan")
# one partial tile, the tile edge, the first halo that crosses a tile, two and three tiles, the two real-time shapes (203 = 12
# tiles + 11 frames)
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 47, 100, 203)

SHIPPED_SPLIT_BELOW = dict(NV.SPLIT_BELOW)
SHIPPED_TORCH_FASTER = dict(NV.LAYER_TORCH_FASTER)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("L", LENGTHS)
def test_parity(dev, L):
    assert NV.split_tile(D, HC) == T
    weights = _weights(10)
    x, cond, d = _inputs(np.random.default_rng(1000 + L), 2, L)
    assert not np.array_equal(x[0], x[1])
    ref = O.layer(x, cond, d, weights)
    s0 = NV.CALLS["split"]
    got = _np(NV.diff_layer(*_t((x, cond, d), dev), _t(weights, dev), form="split"))
    assert NV.CALLS["split"] == s0 + 1
    _check("split L %d" % L, got, ref, _bar(_torch_layer(x, cond, d, weights), ref))


# ---- the same bits as the tiled form ----------------------------------------------------------------------------------------------

def _both_forms(x, cond, d, wt, device):
    """(split, tiled): ``out`` and an explicit ``ws`` of exactly the form's size hold NaN before the call"""
    B, L = x.shape[:2]
    lib = _ffi.lib()
    got = []
    for form, size in (("split", lib.ddsp_hip_naive_v2_layer_split_workspace_bytes), ("tiled", lib.ddsp_hip_naive_v2_layer_workspace_bytes)):
        xt, ct, dt = _t((x, cond, d), device)
        ws = torch.full((size(B, L, D) // 4,), NAN, device=device)
        y = NV.diff_layer(xt, ct, dt, wt, out=torch.full_like(xt, NAN), ws=ws, form=form)
        assert torch.isfinite(y).all(), form
        got.append(y)
    return got


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B,L", [(1, L) for L in LENGTHS] + [(3, 33)])
@pytest.mark.parametrize("scale", (1.0, 100.0))
def test_same_bits_as_the_tiled_form(dev, scale, B, L):
    """scale 100: x and cond a hundred times larger, so that the gate and the stencil saturate (expf overflows, the sigmoids are
    0 or 1)"""
    weights = _weights(20)
    x, cond, d = _inputs(np.random.default_rng(2000 + L + B), B, L)
    if B > 1:
        _rows_differ(x)
    x, cond = (np.float32(scale) * x).astype(np.float32), (np.float32(scale) * cond).astype(np.float32)
    if scale > 1.0:
        assert np.abs(O.pre_glu(x, cond, d, weights)[..., 2 * D:]).max() > 100.0
    split, tiled = _both_forms(x, cond, d, _t(weights, dev), dev)
    assert torch.equal(split, tiled)


# ---- the stack and the packed cache -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_stack_and_packed_cache(dev):
    B, L = 2, 17
    layers = _layers(250, 3)
    lt = [(_t(w, dev), _t(p, dev)) for w, p in layers]
    rng = np.random.default_rng(251)
    x, cond, _ = _inputs(rng, B, L)
    s = rng.standard_normal((B, D)).astype(np.float32)
    xt, ct, st = _t((x, cond, s), dev)
    ref = O.stack(x, cond, s, layers)
    bar = _bar(_torch_stack(x, cond, s, layers), ref)
    p0, s0, h0 = NV.PACKS["count"], NV.CALLS["split"], NV.CALLS["hip"]
    y = NV.diff_stack(xt, ct, st, lt, form="split")
    assert NV.PACKS["count"] == p0 + 3 and (NV.CALLS["split"], NV.CALLS["hip"]) == (s0 + 3, h0 + 3)
    assert torch.equal(xt.cpu(), torch.from_numpy(x)) and torch.equal(ct.cpu(), torch.from_numpy(cond))   # never written
    _check("split stack", _np(y), ref, bar)
    tiled = NV.diff_stack(xt, ct, st, lt, form="tiled")
    assert torch.equal(y, tiled)
    assert NV.PACKS["count"] == p0 + 3                 # one table for both forms
    assert (NV.CALLS["split"], NV.CALLS["hip"]) == (s0 + 3, h0 + 6)
    # an in-place write bumps _version: the table is rebuilt once and both forms follow the new weight (one utterance, one layer)
    lt[1][0][6].mul_(-1.5)
    changed = tuple(a if i != 6 else a * np.float32(-1.5) for i, a in enumerate(layers[1][0]))
    d = torch.from_numpy(O.project(s, layers[1][1]).astype(np.float32)).to(dev)
    y2 = NV.diff_layer(xt[:1], ct[:1], d[:1], lt[1][0], form="split")
    assert NV.PACKS["count"] == p0 + 4
    assert torch.equal(y2, NV.diff_layer(xt[:1], ct[:1], d[:1], lt[1][0])) and NV.PACKS["count"] == p0 + 4   # the default: tiled
    assert (NV.CALLS["split"], NV.CALLS["hip"]) == (s0 + 4, h0 + 8)
    ref2 = O.layer(x[:1], cond[:1], d[:1].cpu().numpy(), changed)
    bar2 = _bar(_torch_layer(x[:1], cond[:1], d[:1].cpu().numpy(), changed), ref2)
    assert np.abs(ref2 - O.layer(x[:1], cond[:1], d[:1].cpu().numpy(), layers[1][0])).max() > 100 * bar2
    _check("split, new weight", _np(y2), ref2, bar2)
    for bad in (dict(form="flat"), dict(form=None), dict(form="split", out=xt)):
        with pytest.raises(ValueError):
            NV.diff_layer(xt, ct, d, lt[0][0], **bad)
    with pytest.raises(ValueError):
        NV.diff_stack(xt, ct, st, lt, form="flat")


# ---- range and refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_range_and_refusals(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    outside = ((256, 128), (512, 256), (0, 0), (-512, 128), (512, -128))
    assert lib.ddsp_hip_naive_v2_layer_split_tile(D, HC) == T == NV.split_tile(D, HC)
    assert [lib.ddsp_hip_naive_v2_layer_split_tile(d, h) for d, h in outside] == [0] * 5
    ws_bytes = lib.ddsp_hip_naive_v2_layer_split_workspace_bytes
    assert ws_bytes(2, 6, D) == 5 * 2 * 6 * D * 4 and ws_bytes(0, 6, D) == 0
    assert ws_bytes(4096, 16, D) == 5 * 4096 * 16 * D * 4 and ws_bytes(1, 65536, D) == 5 * 65536 * D * 4
    assert [ws_bytes(*a) for a in ((-1, 6, D), (2, 0, D), (2, 2 ** 30 + 1, D), (2, 6, 256), (4097, 1, D), (4096, 17, D),
                                   (1, 65537, D))] == [0] * 7
    weights = _weights(90)
    w = [torch.from_numpy(a) for a in weights]
    need = lib.ddsp_hip_naive_v2_layer_pack_bytes(D, HC)
    tab = torch.zeros(need // 4)
    assert lib.ddsp_hip_naive_v2_layer_pack(*[a.data_ptr() for a in w], D, HC, tab.data_ptr(), need) == 0
    L = 6
    gen = torch.Generator().manual_seed(1)
    x, cond, d = torch.randn(2, L, D, generator=gen), torch.randn(2, L, HC, generator=gen), torch.randn(2, D, generator=gen)
    y = torch.full((2, L, D), 7.0)
    wsn = ws_bytes(2, L, D)
    ws = torch.zeros(wsn // 4)

    def call(entry=lib.ddsp_hip_naive_v2_layer_split, **kw):
        return entry(*[kw.get(n, v) for n, v in (
            ("x", x.data_ptr()), ("cond", cond.data_ptr()), ("d", d.data_ptr()), ("y", y.data_ptr()), ("t", tab.data_ptr()),
            ("tb", need), ("ws", ws.data_ptr()), ("wb", wsn), ("B", 2), ("L", L), ("D", D), ("H", HC), ("st", None))])

    refused = (({"D": 256}, -3), ({"H": 256}, -3), ({"D": 0, "H": 0}, -3), ({"L": 0}, -1), ({"L": -1}, -1),
               ({"L": 2 ** 30 + 1}, -3), ({"B": -1}, -1), ({"tb": need - 4}, -4), ({"wb": wsn - 4}, -4), ({"x": None}, -1),
               ({"cond": None}, -1), ({"d": None}, -1), ({"y": None}, -1), ({"t": None}, -1), ({"ws": None}, -1),
               ({"y": x.data_ptr()}, -1), ({"y": cond.data_ptr()}, -1))
    tiled_wsn = lib.ddsp_hip_naive_v2_layer_workspace_bytes(2, L, D)
    for kw, code in refused:
        assert call(**kw) == code, kw
        tiled_kw = dict(kw, wb=tiled_wsn - 4 if "wb" in kw else tiled_wsn)         # its own workspace size
        assert call(lib.ddsp_hip_naive_v2_layer, **tiled_kw) == code, kw           # as the tiled entry refuses them
        assert (y == 7.0).all() and (ws == 0.0).all(), kw                          # refused before any launch
    # the tiled form's workspace (2 B L D floats) is short for the split form
    assert call(wb=tiled_wsn) == -4 and (y == 7.0).all()
    # past the cap of 4096 tiles: a matter of shape, whatever the buffers hold
    huge = 5 * 4097 * 16 * D * 4
    for kw in ({"B": 4097, "L": 1}, {"B": 4097, "L": 16}, {"B": 4096, "L": 17}, {"B": 1, "L": 65537}, {"B": 2, "L": 32769}):
        assert call(wb=huge, **kw) == -3, kw
        assert (y == 7.0).all() and (ws == 0.0).all(), kw
    assert call(B=0, x=None, y=None, ws=None, wb=0) == 0 and (y == 7.0).all()      # a no-op
    assert call() == 0
    ref = O.layer(x.numpy(), cond.numpy(), d.numpy(), weights)
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    y2 = torch.full((2, L, D), 7.0)
    assert call(lib.ddsp_hip_naive_v2_layer, y=y2.data_ptr()) == 0 and torch.equal(y, y2)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_python_refuses_a_call_past_the_cap(dev):
    wt = _t(_weights(90), dev)
    h0 = NV.CALLS["hip"]
    for B, L in ((4097, 1), (1, 65537)):
        x, cond, d = torch.zeros(B, L, D), torch.zeros(B, L, HC), torch.zeros(B, D)
        with pytest.raises(ValueError):
            NV.diff_layer(x, cond, d, wt, form="split")
        with pytest.raises(ValueError):
            NV.diff_stack(x, cond, d, [(wt, _t(O.seeded_projection(D, 91), dev))], form="split")
    assert NV.CALLS["hip"] == h0
    with pytest.raises(RuntimeError, match="code -4"):     # the tiled form's workspace is short: DDSP_HIP_EWS from the entry point
        NV.diff_layer(torch.zeros(1, 3, D), torch.zeros(1, 3, HC), torch.zeros(1, D), wt, form="split", ws=torch.zeros(2 * 3 * D))


@pytest.mark.gpu
def test_at_the_cap():
    """B x tiles = 4096 at L = 1, utterance b = pool[b % 251] (251 is prime and 4096 mod 251 = 80: a wrong base or stride moves an
    utterance onto another pool entry), compared bitwise with the pool's own run, which the oracle checks; 4097 is refused"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    POOL, B, L = 251, 4096, 1
    weights = _weights(80)
    wt = _t(weights, device)
    xp, cp, dp = _inputs(np.random.default_rng(81), POOL, L)
    ref = O.layer(xp, cp, dp, weights)
    xpool, cpool, dpool = _t((xp, cp, dp), device)
    ypool = NV.diff_layer(xpool, cpool, dpool, wt, form="split")
    _check("pool", _np(ypool), ref, _bar(_torch_layer(xp, cp, dp, weights), ref))
    _rows_differ(ref)
    idx = torch.arange(B + 1, device=device) % POOL
    x, cond, d = xpool[idx].contiguous(), cpool[idx].contiguous(), dpool[idx].contiguous()
    y = NV.diff_layer(x[:B], cond[:B], d[:B], wt, out=torch.full_like(x[:B], NAN), form="split")
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx[:B]])
    with pytest.raises(ValueError):
        NV.diff_layer(x, cond, d, wt, form="split")
    NV.release_workspace()


# ---- dispatch -------------------------------------------------------------------------------------------------------------------

def test_choose_form(monkeypatch):
    monkeypatch.setattr(NV, "LAYER_TORCH_FASTER", {512: 27584})
    monkeypatch.setattr(NV, "SPLIT_BELOW", {})
    # an empty table: today's routing
    assert [NV.choose_form(D, B, L) for B, L in ((1, 100), (48, 172), (32, 862))] == [None, None, "tiled"]
    assert NV.choose_form(D, 1, 27583) is None and NV.choose_form(D, 1, 27584) == "tiled"
    monkeypatch.setattr(NV, "SPLIT_BELOW", {512: 4096})
    assert [NV.choose_form(D, B, L) for B, L in ((1, 100), (1, 203), (48, 172), (32, 862))] == ["split", "split", None, "tiled"]
    assert NV.choose_form(D, 1, 4095) == "split" and NV.choose_form(D, 1, 4096) is None
    # over the cap of 4096 tiles never "split", whatever the table says
    monkeypatch.setattr(NV, "SPLIT_BELOW", {512: 10 ** 9})
    assert NV.choose_form(D, 4096, 1) == "split" and NV.choose_form(D, 4097, 1) is None
    assert NV.choose_form(D, 1, 65536) == "split" and NV.choose_form(D, 1, 65537) == "tiled"
    assert NV.choose_form(D, 4096, 16) == "split" and NV.choose_form(D, 4096, 17) == "tiled"
    monkeypatch.setattr(NV, "LAYER_TORCH_FASTER", {})
    assert NV.choose_form(D, 4097, 1) == "tiled"


def _counts():
    return NV.CALLS["split"], NV.CALLS["hip"], NV.CALLS["reference"]


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_hook_takes_the_split_form_below_the_bound(dev, monkeypatch):
    M = _standin_module("reflow.naive_v2_diff")
    monkeypatch.setitem(sys.modules, "reflow.naive_v2_diff", M)
    monkeypatch.setattr(NV, "LAYER_TORCH_FASTER", {512: 27584})
    layer_fwd, net_fwd = M.NaiveV2DiffLayer.forward, M.NaiveV2Diff.forward
    torch.manual_seed(8)
    layers = [O.load(M.NaiveV2DiffLayer(D, HC), _weights(330 + i), O.seeded_projection(D, 340 + i)) for i in range(3)]
    net = M.NaiveV2Diff(8, D, HC, layers=layers).eval()
    L = 5
    spec, step, cond = torch.randn(1, 1, 8, L), torch.tensor([7.0]), torch.randn(1, HC, L)
    x, st = torch.randn(1, D, L), torch.randn(1, D, 1)
    with torch.no_grad():
        try:
            assert M in NV.patch_reference_naive_v2()
            # an empty table: 5 frames are torch's, as today
            monkeypatch.setattr(NV, "SPLIT_BELOW", {})
            c0 = _counts()
            want = net(spec, step, cond)
            assert _counts() == (c0[0], c0[1], c0[2] + 3)
            # the tiled hook: today's behaviour with the crossover table out of the way
            monkeypatch.setattr(NV, "LAYER_TORCH_FASTER", {})
            c0 = _counts()
            tiled, tiled_one = net(spec, step, cond), layers[0](x, cond, st)
            assert _counts() == (c0[0], c0[1] + 4, c0[2])
            monkeypatch.setattr(NV, "LAYER_TORCH_FASTER", {512: 27584})
            monkeypatch.setattr(NV, "SPLIT_BELOW", {512: 4096})
            c0 = _counts()
            got = net(spec, step, cond)
            assert _counts() == (c0[0] + 3, c0[1] + 3, c0[2])
            one = layers[0](x, cond, st)
            assert _counts() == (c0[0] + 4, c0[1] + 4, c0[2])
            assert torch.equal(got, tiled) and torch.equal(one, tiled_one)
            # at and above the bound the size is torch's again
            monkeypatch.setattr(NV, "SPLIT_BELOW", {512: L})
            c0 = _counts()
            net(spec, step, cond)
            assert _counts() == (c0[0], c0[1], c0[2] + 3)
            monkeypatch.setattr(NV, "SPLIT_BELOW", {512: 4096})
            # autocast and a needed gradient still go to the reference
            with torch.autocast("cpu", dtype=torch.bfloat16):
                c0 = _counts()
                layers[0](x, cond, st)
                assert _counts() == (c0[0], c0[1], c0[2] + 1)
            with torch.enable_grad():
                c0 = _counts()
                yg = layers[0](x.clone().requires_grad_(True), cond, st)
                assert _counts() == (c0[0], c0[1], c0[2] + 1) and yg.requires_grad
        finally:
            NV.unpatch_reference_naive_v2()
        assert M.NaiveV2DiffLayer.forward is layer_fwd and M.NaiveV2Diff.forward is net_fwd
        assert "_reference_forward" not in M.NaiveV2DiffLayer.__dict__ and "_reference_forward" not in M.NaiveV2Diff.__dict__
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-5 * float(want.abs().max())


def test_hook_keeps_host_tensors_on_the_reference(monkeypatch):
    monkeypatch.setattr(NV, "SPLIT_BELOW", {512: 4096})
    layer = S.DiffLayer(D, HC).eval()
    inputs = torch.randn(1, D, 3), torch.randn(1, HC, 3), torch.randn(1, D, 1)
    with torch.no_grad():
        c0 = _counts()
        got = layer(*inputs)
        assert _counts() == (c0[0], c0[1], c0[2] + 1)
        assert torch.equal(got, layer.reference_forward(*inputs))


# ---- the committed table ----------------------------------------------------------------------------------------------------------

def _choose(split_below, torch_faster, d, B, L):
    if d in split_below and NV.split_in_range(B, L) and B * L < split_below[d]:
        return "split"
    return "torch" if d in torch_faster and (torch_faster[d] is None or B * L < torch_faster[d]) else "tiled"


def test_split_table_agrees_with_the_committed_measurements():
    """every single-layer case of profiles/naive_v2_split_latency.json is routed by the shipped tables to whichever of the three
    sides was measured fastest there; without the file the table is empty"""
    if not os.path.exists(PROFILE):
        assert SHIPPED_SPLIT_BELOW == {}
        return
    with open(PROFILE) as f:
        doc = json.load(f)
    assert doc["Hc"] == HC and doc["tile_split"] == T
    cases = [c for c in doc["cases"] if c["case"] == "layer"]
    assert {(c["B"], c["L"]) for c in cases} == {(1, 100), (1, 203), (1, 862), (4, 203), (48, 172)}
    assert set(SHIPPED_SPLIT_BELOW) <= {c["D"] for c in cases}
    for c in cases:
        times = {"torch": c["torch_ms"], "tiled": c["tiled_ms"], "split": c["split_ms"]}
        fastest = min(times, key=times.get)
        assert c["fastest"] == fastest
        assert _choose(SHIPPED_SPLIT_BELOW, SHIPPED_TORCH_FASTER, c["D"], c["B"], c["L"]) == fastest, (c["B"], c["L"], times)
    for d, bound in SHIPPED_SPLIT_BELOW.items():
        mine = sorted((c["frames"], c["fastest"]) for c in cases if c["D"] == d)
        assert mine[0][1] == "split"                   # an entry only if the split form is the fastest at 1 x 100
        lost = [n for n, side in mine if side != "split"]
        assert bound == (lost[0] if lost else mine[-1][0] + 1)


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _stack_case(device, L=100, n=6):
    layers = _layers(370, n)
    lt = [(_t(w, device), _t(p, device)) for w, p in layers]
    gen = torch.Generator().manual_seed(4)
    x, cond, s = torch.randn(1, L, D, generator=gen), torch.randn(1, L, HC, generator=gen), torch.randn(1, D, generator=gen)
    return layers, lt, x.to(device), cond.to(device), s.to(device)


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical_and_allocates_only_its_buffers():
    """the 6-layer split stack at 1 x 100 is a chain of launches on the caller's stream: a capture of it has no parallel branches"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    layers, lt, x, cond, s = _stack_case(device)
    eager = NV.diff_stack(x, cond, s, lt, form="split")    # the warm call packs the tables, stacks the projections, sizes the workspace
    xn, cn, sn = x.cpu().numpy(), cond.cpu().numpy(), s.cpu().numpy()
    ref = O.stack(xn, cn, sn, layers)
    _check("split stack of 6 at 1 x 100", _np(eager), ref, _bar(_torch_stack(xn, cn, sn, layers), ref))
    assert torch.equal(eager, NV.diff_stack(x, cond, s, lt, form="tiled"))
    torch.cuda.synchronize()
    p0 = NV.PACKS["count"]
    nbytes = -(-(x.numel() * 4) // 512) * 512
    d_bytes = -(-(6 * s.numel() * 4) // 512) * 512
    before = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    held = NV.diff_stack(x, cond, s, lt, form="split")
    assert torch.cuda.memory_allocated(device) - before == nbytes                # the result stays
    assert torch.cuda.max_memory_allocated(device) - before <= 2 * nbytes + 2 * d_bytes   # + one hand-over buffer and d
    assert NV.PACKS["count"] == p0
    del held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = NV.diff_stack(x, cond, s, lt, form="split")
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
    _, lt, x, cond, s = _stack_case(device, L=203, n=1)
    d = s.clone()
    eager = NV.diff_layer(x, cond, d, lt[0][0], form="split")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    big = torch.randn(4096, 4096, device=device)
    xs = torch.zeros_like(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big @ big * 1e-2                     # keeps the side stream busy while the host runs ahead
        xs.copy_(x)
        y = NV.diff_layer(xs, cond, d, lt[0][0], form="split")
    side.synchronize()
    assert torch.equal(y, eager)
