"""The channel-split form of the WaveNet residual layer (ddsp_svc_amd.wavenet with form="split", csrc/wavenet_split.h): two launches
with a frame tile of 16, on the emulator and the GPU against the float64 oracle and, bit for bit, against the tiled form
(csrc/wavenet_layer.h), whose sums it repeats in the same order; the zero padding of x + d, the stack, the range, the C ABI, the
three-way dispatch (split form, tiled form, torch) and the committed crossover table.

The parity bar is test_wavenet.py's: 4 e_torch + 1e-7 rms(oracle), e_torch the error of the float32 torch op chain on the CPU on
the same inputs, separately for x_out and skip.  Every case prints its err / bar."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import wavenet_oracle as O
from tests import wavenet_standin as S
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_wavenet import _bars, _check, _inputs, _rows_differ, _t, _torch_layer, _torch_stack

from ddsp_svc_amd import _ffi, wavenet as WN  # noqa: E402

H = 256
SHAPES = ((384, H), (512, H))
TILE = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "wavenet_split_latency.json")
NAN = float("nan")
# a partial tile, the tile edge, the 1-frame halo crossing a tile, two tiles and the two real-time shapes (203 = 12 tiles + 11 frames)
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 100, 203)

SHIPPED_SPLIT_BELOW = dict(WN.SPLIT_BELOW)
SHIPPED_TORCH_FASTER = dict(WN.LAYER_TORCH_FASTER)


def _np(pair):
    return tuple(a.cpu().numpy().astype(np.float64) for a in pair)


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("C,Hc", SHAPES)
def test_parity(dev, C, Hc, T):
    assert WN.split_tile(C, Hc) == TILE
    weights = O.seeded_weights(C, Hc, 10)
    x, cond, d = _inputs(np.random.default_rng(1000 * C + T), 2, C, T)
    assert not np.array_equal(x[0], x[1])
    ref = O.layer(x, cond, d, weights)
    s0, h0 = WN.CALLS["split"], WN.CALLS["hip"]
    got = _np(WN.residual_layer(*_t((x, cond, d), dev), _t(weights, dev), form="split"))
    assert (WN.CALLS["split"], WN.CALLS["hip"]) == (s0 + 1, h0 + 1)
    _check("split C %d T %d" % (C, T), got, ref, _bars(_torch_layer(x, cond, d, weights), ref))


# ---- the same bits as the tiled form ----------------------------------------------------------------------------------------------

def _both_forms(x, cond, d, wt, device, preset=None):
    """((x_out, skip) of the split form, of the tiled form): ``out``, ``skip`` and an explicit ``ws`` of exactly the form's size
    hold NaN before the call; with ``preset``, ``skip`` holds it and the call accumulates"""
    B, C, T = x.shape
    got = []
    for form in ("split", "tiled"):
        xt, ct, dt = _t((x, cond, d), device)
        kw = {}
        if form == "split":
            kw["ws"] = torch.full((_ffi.lib().ddsp_hip_wavenet_layer_split_workspace_bytes(B, T, C) // 4,), NAN, device=device)
            assert kw["ws"].numel() == B * T * C
        skip = torch.full_like(xt, NAN) if preset is None else _t((preset,), device)[0]
        y, s = WN.residual_layer(xt, ct, dt, wt, out=torch.full_like(xt, NAN), skip=skip, accumulate=preset is not None, form=form,
                                 **kw)
        assert s is skip and torch.isfinite(y).all() and torch.isfinite(s).all(), form
        got.append((y, s))
    return got


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B,T", [(1, T) for T in LENGTHS] + [(3, 33)])
@pytest.mark.parametrize("scale", (1.0, 100.0))
@pytest.mark.parametrize("C,Hc", SHAPES)
def test_same_bits_as_the_tiled_form(dev, C, Hc, scale, B, T):
    """scale 100: x and cond a hundred times larger, so that sigmoid and tanh saturate (expf overflows)"""
    weights = O.seeded_weights(C, Hc, 20)
    x, cond, d = _inputs(np.random.default_rng(2000 * C + 8 * T + B), B, C, T)
    if B > 1:
        _rows_differ(x)
    x, cond = (np.float32(scale) * x).astype(np.float32), (np.float32(scale) * cond).astype(np.float32)
    if scale > 1.0:
        assert np.abs(O.z_of(x, cond, d, weights)).max() > 100.0
    split, tiled = _both_forms(x, cond, d, _t(weights, dev), dev)
    assert torch.equal(split[0], tiled[0]) and torch.equal(split[1], tiled[1])


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("C,Hc", SHAPES)
def test_accumulate_adds_the_same_bits_onto_a_preloaded_skip(dev, C, Hc):
    weights = O.seeded_weights(C, Hc, 30)
    wt = _t(weights, dev)
    for B, T in ((2, 17),):                            # two utterances of two tiles, the second tile one frame
        rng = np.random.default_rng(3000 + C + T)
        x, cond, d = _inputs(rng, B, C, T)
        preset = rng.standard_normal((B, C, T)).astype(np.float32)
        plain = _both_forms(x, cond, d, wt, dev)[0]
        split, tiled = _both_forms(x, cond, d, wt, dev, preset=preset)
        assert torch.equal(split[0], tiled[0]) and torch.equal(split[1], tiled[1])
        assert torch.equal(split[0], plain[0]) and torch.equal(split[1], _t((preset,), dev)[0] + plain[1])


# ---- edges: the convolution pads its own input ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("C,Hc", SHAPES)
def test_x_plus_d_is_zero_outside_the_sequence(dev, C, Hc):
    weights = O.seeded_weights(C, Hc, 20)
    wt = _t(weights, dev)
    rng = np.random.default_rng(21 + C)
    for T in (TILE, TILE + 1):
        x = np.zeros((1, C, T), np.float32)
        cond = rng.standard_normal((1, Hc, T)).astype(np.float32)
        d = (10.0 * np.sign(rng.standard_normal((1, C)))).astype(np.float32)
        ref = O.layer(x, cond, d, weights)
        bars = _bars(_torch_layer(x, cond, d, weights), ref)
        got = _np(WN.residual_layer(*_t((x, cond, d), dev), wt, form="split"))
        wrong = O.layer(x, cond, d, weights, pad_with_d=True)
        for f in (0, T - 1):
            edge = lambda pair: tuple(a[:, :, f] for a in pair)
            _check("split C %d T %d frame %d" % (C, T, f), edge(got), edge(ref), bars)
            for w, r, bar in zip(edge(wrong), edge(ref), bars):
                assert np.abs(w - r).max() > 10 * bar, (T, f)                       # the case can fail
        _check("split C %d T %d" % (C, T), got, ref, bars)


# ---- the stack and the packed cache -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("C,Hc", SHAPES)
def test_stack_and_packed_cache(dev, C, Hc):
    B, T = 2, 17
    layers = [(O.seeded_weights(C, Hc, 250 + i), O.seeded_projection(C, 260 + i)) for i in range(3)]
    lt = [(_t(w, dev), _t(p, dev)) for w, p in layers]
    rng = np.random.default_rng(251)
    x, cond, _ = _inputs(rng, B, C, T)
    s = rng.standard_normal((B, C)).astype(np.float32)
    xt, ct, st = _t((x, cond, s), dev)
    ref = O.stack(x, cond, s, layers)
    bars = _bars(_torch_stack(x, cond, s, layers), ref)
    p0, s0, h0 = WN.PACKS["count"], WN.CALLS["split"], WN.CALLS["hip"]
    y, total = WN.residual_stack(xt, ct, st, lt, form="split")
    assert WN.PACKS["count"] == p0 + 3 and (WN.CALLS["split"], WN.CALLS["hip"]) == (s0 + 3, h0 + 3)
    assert torch.equal(xt.cpu(), torch.from_numpy(x)) and torch.equal(ct.cpu(), torch.from_numpy(cond))   # never written
    assert torch.equal(st.cpu(), torch.from_numpy(s))
    _check("split stack C %d" % C, _np((y, total)), ref, bars)
    y2, total2 = WN.residual_stack(xt, ct, st, lt, form="tiled")
    assert torch.equal(y, y2) and torch.equal(total, total2)
    assert WN.PACKS["count"] == p0 + 3                 # one table for both forms
    assert (WN.CALLS["split"], WN.CALLS["hip"]) == (s0 + 3, h0 + 6)
    # an in-place write bumps _version: the table is rebuilt once and both forms follow the new weight (one utterance, one layer)
    lt[1][0][4].mul_(-1.5)
    changed = tuple(a if i != 4 else a * np.float32(-1.5) for i, a in enumerate(layers[1][0]))
    dn = O.project(s, layers[1][1]).astype(np.float32)[:1]
    d = torch.from_numpy(dn).to(dev)
    got = WN.residual_layer(xt[:1], ct[:1], d, lt[1][0], form="split")
    assert WN.PACKS["count"] == p0 + 4
    again = WN.residual_layer(xt[:1], ct[:1], d, lt[1][0])                         # the default: tiled
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]) and WN.PACKS["count"] == p0 + 4
    assert (WN.CALLS["split"], WN.CALLS["hip"]) == (s0 + 4, h0 + 8)
    ref2 = O.layer(x[:1], cond[:1], dn, changed)
    bars2 = _bars(_torch_layer(x[:1], cond[:1], dn, changed), ref2)
    assert np.abs(ref2[1] - O.layer(x[:1], cond[:1], dn, layers[1][0])[1]).max() > 100 * bars2[1]
    _check("split, new weight", _np(got), ref2, bars2)
    for bad in (dict(form="flat"), dict(form=None), dict(form="split", out=xt), dict(form="split", skip=xt)):
        with pytest.raises(ValueError):
            WN.residual_layer(xt, ct, torch.zeros(B, C, device=dev), lt[0][0], **bad)
    for bad in ("flat", None):
        with pytest.raises(ValueError):
            WN.residual_stack(xt, ct, st, lt, form=bad)
    assert (WN.CALLS["split"], WN.CALLS["hip"]) == (s0 + 4, h0 + 8)


# ---- range and refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_range_and_refusals(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    C = 384
    outside = ((256, 256), (384, 128), (0, 0), (-384, 256), (384, -256))
    assert [lib.ddsp_hip_wavenet_layer_split_tile(c, h) for c, h in SHAPES] == [TILE, TILE]
    assert [WN.split_tile(c, h) for c, h in SHAPES] == [TILE, TILE]
    assert [lib.ddsp_hip_wavenet_layer_split_tile(c, h) for c, h in outside] == [0] * 5
    ws_bytes = lib.ddsp_hip_wavenet_layer_split_workspace_bytes
    assert ws_bytes(2, 6, C) == 2 * 6 * C * 4 and ws_bytes(3, 33, 512) == 3 * 33 * 512 * 4
    assert ws_bytes(4096, 16, C) == 4096 * 16 * C * 4 and ws_bytes(1, 65536, 512) == 65536 * 512 * 4
    assert [ws_bytes(*a) for a in ((0, 6, C), (-1, 6, C), (2, 0, C), (2, -3, C), (2, 6, 256), (2, 6, 0), (4097, 1, C), (4096, 17, C),
                                   (1, 65537, C), (2 ** 40, 2 ** 40, C))] == [0] * 10
    weights = O.seeded_weights(C, H, 90)
    w = [torch.from_numpy(a) for a in weights]
    need = lib.ddsp_hip_wavenet_layer_pack_bytes(C, H)
    tab = torch.zeros(need // 4)
    assert lib.ddsp_hip_wavenet_layer_pack(*[a.data_ptr() for a in w], C, H, tab.data_ptr(), need) == 0
    T = 6
    gen = torch.Generator().manual_seed(1)
    x, cond, d = torch.randn(2, C, T, generator=gen), torch.randn(2, H, T, generator=gen), torch.randn(2, C, generator=gen)
    y, s = torch.full((2, C, T), 7.0), torch.full((2, C, T), 7.0)
    wsn = ws_bytes(2, T, C)
    ws = torch.zeros(wsn // 4)
    values = dict(x=x.data_ptr(), cond=cond.data_ptr(), d=d.data_ptr(), y=y.data_ptr(), s=s.data_ptr(), t=tab.data_ptr(), tb=need,
                  ws=ws.data_ptr(), wb=wsn, B=2, T=T, C=C, H=H, mode=0, st=None)

    def split(**kw):
        return lib.ddsp_hip_wavenet_layer_split(*[kw.get(n, values[n]) for n in (
            "x", "cond", "d", "y", "s", "t", "tb", "ws", "wb", "B", "T", "C", "H", "mode", "st")])

    def tiled(**kw):
        return lib.ddsp_hip_wavenet_layer(*[kw.get(n, values[n]) for n in (
            "x", "cond", "d", "y", "s", "t", "tb", "B", "T", "C", "H", "mode", "st")])

    untouched = lambda: bool((y == 7.0).all() and (s == 7.0).all() and (ws == 0.0).all())
    shared = (({"C": 256}, -3), ({"H": 128}, -3), ({"C": 0, "H": 0}, -3), ({"T": 0}, -1), ({"T": -1}, -1), ({"T": 2 ** 40 + 1}, -3),
              ({"B": -1}, -1), ({"tb": need - 4}, -4), ({"x": None}, -1), ({"cond": None}, -1), ({"d": None}, -1), ({"y": None}, -1),
              ({"s": None}, -1), ({"t": None}, -1), ({"y": x.data_ptr()}, -1), ({"s": x.data_ptr()}, -1), ({"s": y.data_ptr()}, -1),
              ({"mode": 2}, -1), ({"mode": -1}, -1),
              # the order of the checks: an argument error before the shape, the shape before a null, a null before a short table
              ({"T": 0, "C": 256}, -1), ({"mode": 2, "C": 256}, -1), ({"C": 256, "x": None}, -3), ({"x": None, "tb": need - 4}, -1))
    for kw, code in shared:
        assert split(**kw) == code, kw
        assert tiled(**kw) == code, kw                                             # as the tiled entry refuses them
        assert untouched(), kw                                                     # refused before any launch
    for kw, code in (({"wb": wsn - 4}, -4), ({"wb": 0}, -4), ({"ws": None}, -1), ({"ws": None, "wb": 0}, -1),
                     ({"ws": None, "C": 256}, -3)):
        assert split(**kw) == code, kw
        assert untouched(), kw
    # past the cap of 4096 tiles: a matter of shape, whatever the buffers are
    huge = 4097 * 16 * 512 * 4
    for kw in ({"B": 4097, "T": 1}, {"B": 4097, "T": 16}, {"B": 4096, "T": 17}, {"B": 1, "T": 65537}, {"B": 2, "T": 32769}):
        for buffers in ({"wb": huge}, {"wb": 0}, {"ws": None}, {"x": None, "y": None, "t": None}):
            assert split(**kw, **buffers) == -3, (kw, buffers)
            assert untouched(), kw
    assert split(B=0, x=None, y=None, ws=None, wb=0) == 0 and untouched()          # a no-op
    assert tiled(B=0, x=None, y=None) == 0 and untouched()
    assert split() == 0
    ref = O.layer(x.numpy(), cond.numpy(), d.numpy(), weights)
    assert np.abs(y.numpy() - ref[0]).max() <= 1e-5 * np.abs(ref[0]).max()
    assert np.abs(s.numpy() - ref[1]).max() <= 1e-5 * np.abs(ref[1]).max()
    y2, s2 = torch.full((2, C, T), 7.0), torch.full((2, C, T), 7.0)
    assert tiled(y=y2.data_ptr(), s=s2.data_ptr()) == 0 and torch.equal(y, y2) and torch.equal(s, s2)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_python_refuses_a_call_past_the_cap(dev):
    C = 384
    wt = _t(O.seeded_weights(C, H, 90), dev)
    proj = _t(O.seeded_projection(C, 91), dev)
    calls = dict(WN.CALLS)
    for B, T in ((4097, 1), (1, 65537)):
        x, cond, d = torch.zeros(B, C, T), torch.zeros(B, H, T), torch.zeros(B, C)
        assert not WN.split_in_range(B, T)
        with pytest.raises(ValueError):
            WN.residual_layer(x, cond, d, wt, form="split")
        with pytest.raises(ValueError):
            WN.residual_stack(x, cond, d, [(wt, proj)], form="split")
    assert WN.split_in_range(4096, 1) and WN.split_in_range(1, 65536) and WN.split_in_range(4096, 16)
    assert WN.CALLS == calls
    with pytest.raises(RuntimeError, match="code -4"):     # a short explicit workspace: DDSP_HIP_EWS from the entry point
        WN.residual_layer(torch.zeros(1, C, 3), torch.zeros(1, H, 3), torch.zeros(1, C), wt, form="split", ws=torch.zeros(3 * C - 1))


@pytest.mark.gpu
def test_at_the_cap():
    """B x tiles = 4096 at T = 1, utterance b = pool[b % 251] (251 is prime and 4096 mod 251 = 80: a wrong base or stride moves an
    utterance onto another pool entry), compared bitwise with the pool's own run, which the oracle checks; 4097 is refused"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    C, POOL, B, T = 384, 251, 4096, 1
    weights = O.seeded_weights(C, H, 80)
    wt = _t(weights, device)
    xp, cp, dp = _inputs(np.random.default_rng(81), POOL, C, T)
    ref = O.layer(xp, cp, dp, weights)
    xpool, cpool, dpool = _t((xp, cp, dp), device)
    ypool, spool = WN.residual_layer(xpool, cpool, dpool, wt, form="split")
    _check("pool", _np((ypool, spool)), ref, _bars(_torch_layer(xp, cp, dp, weights), ref))
    _rows_differ(ref[0])
    idx = torch.arange(B + 1, device=device) % POOL
    x, cond, d = xpool[idx].contiguous(), cpool[idx].contiguous(), dpool[idx].contiguous()
    y, s = WN.residual_layer(x[:B], cond[:B], d[:B], wt, out=torch.full_like(x[:B], NAN), skip=torch.full_like(x[:B], NAN),
                             form="split")
    assert torch.isfinite(y).all() and torch.isfinite(s).all()
    assert torch.equal(y, ypool[idx[:B]]) and torch.equal(s, spool[idx[:B]])
    with pytest.raises(ValueError):
        WN.residual_layer(x, cond, d, wt, form="split")
    WN.release_workspace()


# ---- dispatch -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", (384, 512))
def test_choose_form(monkeypatch, C):
    monkeypatch.setattr(WN, "LAYER_TORCH_FASTER", {C: 27584})
    monkeypatch.setattr(WN, "SPLIT_BELOW", {})
    # an empty table: today's routing
    assert [WN.choose_form(C, B, T) for B, T in ((1, 100), (48, 172), (32, 862))] == [None, None, "tiled"]
    assert WN.choose_form(C, 1, 27583) is None and WN.choose_form(C, 1, 27584) == "tiled"
    monkeypatch.setattr(WN, "SPLIT_BELOW", {C: 4096})
    assert [WN.choose_form(C, B, T) for B, T in ((1, 100), (1, 203), (48, 172), (32, 862))] == ["split", "split", None, "tiled"]
    assert WN.choose_form(C, 1, 4095) == "split" and WN.choose_form(C, 1, 4096) is None
    assert WN.choose_form(896 - C, 1, 100) == "tiled"  # the other C has no entry in either table
    # over the cap of 4096 tiles never "split", whatever the table says
    monkeypatch.setattr(WN, "SPLIT_BELOW", {C: 10 ** 9})
    assert WN.choose_form(C, 4096, 1) == "split" and WN.choose_form(C, 4097, 1) is None
    assert WN.choose_form(C, 1, 65536) == "split" and WN.choose_form(C, 1, 65537) == "tiled"
    assert WN.choose_form(C, 4096, 16) == "split" and WN.choose_form(C, 4096, 17) == "tiled"
    monkeypatch.setattr(WN, "LAYER_TORCH_FASTER", {})
    assert WN.choose_form(C, 4097, 1) == "tiled"


def _counts():
    return WN.CALLS["split"], WN.CALLS["hip"], WN.CALLS["reference"]


def _standin_module(name):
    """a module object with the two class names, whose forwards are the reference's own op chain"""
    mod = types.ModuleType(name)

    class ResidualBlock(S.ResidualBlock):
        forward = S.ResidualBlock.reference_forward

    class WaveNet(S.WaveNet):
        def forward(self, spec, diffusion_step, cond):                              # every layer through its own forward
            x = torch.relu(self.input_projection(spec.squeeze(1)))
            s = self.mlp(self.diffusion_embedding(diffusion_step))
            skips = []
            for layer in self.residual_layers:
                x, sk = layer(x, cond, s)
                skips.append(sk)
            x = torch.sum(torch.stack(skips), dim=0) / float(np.sqrt(len(skips)))
            return self.output_projection(torch.relu(self.skip_projection(x)))[:, None, :, :]

    mod.ResidualBlock, mod.WaveNet = ResidualBlock, WaveNet
    return mod


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_hook_takes_the_split_form_below_the_bound(dev, monkeypatch):
    M = _standin_module("diffusion.wavenet")
    monkeypatch.setitem(sys.modules, "diffusion.wavenet", M)
    monkeypatch.setattr(WN, "LAYER_TORCH_FASTER", {384: 27584})
    block_fwd, net_fwd = M.ResidualBlock.forward, M.WaveNet.forward
    C, T = 384, 5
    torch.manual_seed(8)
    blocks = [S.load(M.ResidualBlock(H, C), O.seeded_weights(C, H, 330 + i), O.seeded_projection(C, 340 + i)) for i in range(3)]
    net = M.WaveNet(8, 3, C, H, blocks=blocks).eval()
    spec, step, cond = torch.randn(1, 1, 8, T), torch.tensor([7.0]), torch.randn(1, H, T)
    x, s = torch.randn(1, C, T), torch.randn(1, C)
    with torch.no_grad():
        try:
            assert WN.patch_reference_wavenet() is M
            assert M.ResidualBlock.forward is not block_fwd and M.WaveNet.forward is not net_fwd
            # an empty table: 5 frames are torch's, as today
            monkeypatch.setattr(WN, "SPLIT_BELOW", {})
            c0 = _counts()
            want = net(spec, step, cond)
            assert _counts() == (c0[0], c0[1], c0[2] + 3)
            # the tiled hook: today's behaviour with the crossover table out of the way
            monkeypatch.setattr(WN, "LAYER_TORCH_FASTER", {})
            c0 = _counts()
            tiled, tiled_one = net(spec, step, cond), blocks[0](x, cond, s)
            assert _counts() == (c0[0], c0[1] + 4, c0[2])
            monkeypatch.setattr(WN, "LAYER_TORCH_FASTER", {384: 27584})
            monkeypatch.setattr(WN, "SPLIT_BELOW", {384: 4096})
            c0 = _counts()
            got = net(spec, step, cond)
            assert _counts() == (c0[0] + 3, c0[1] + 3, c0[2])
            one = blocks[0](x, cond, s)
            assert _counts() == (c0[0] + 4, c0[1] + 4, c0[2])
            assert torch.equal(got, tiled) and torch.equal(one[0], tiled_one[0]) and torch.equal(one[1], tiled_one[1])
            # at and above the bound the size is torch's again
            monkeypatch.setattr(WN, "SPLIT_BELOW", {384: T})
            c0 = _counts()
            net(spec, step, cond)
            blocks[0](x, cond, s)
            assert _counts() == (c0[0], c0[1], c0[2] + 4)
            monkeypatch.setattr(WN, "SPLIT_BELOW", {384: 4096})
            # autocast and a needed gradient still go to the reference
            with torch.autocast("cpu", dtype=torch.bfloat16):
                c0 = _counts()
                blocks[0](x, cond, s)
                assert _counts() == (c0[0], c0[1], c0[2] + 1)
            with torch.enable_grad():
                c0 = _counts()
                yg, _ = blocks[0](x.clone().requires_grad_(True), cond, s)
                assert _counts() == (c0[0], c0[1], c0[2] + 1) and yg.requires_grad
        finally:
            WN.unpatch_reference_wavenet()
        assert M.ResidualBlock.forward is block_fwd and M.WaveNet.forward is net_fwd
        assert "_reference_forward" not in M.ResidualBlock.__dict__ and "_reference_forward" not in M.WaveNet.__dict__
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-5 * float(want.abs().max())


def test_hook_keeps_host_tensors_on_the_reference(monkeypatch):
    monkeypatch.setattr(WN, "SPLIT_BELOW", {384: 4096})
    block = S.ResidualBlock(H, 384).eval()
    inputs = torch.randn(1, 384, 3), torch.randn(1, H, 3), torch.randn(1, 384)
    with torch.no_grad():
        c0 = _counts()
        got = block(*inputs)
        assert _counts() == (c0[0], c0[1], c0[2] + 1)
        for g, w in zip(got, block.reference_forward(*inputs)):
            assert torch.equal(g, w)


# ---- the committed table ----------------------------------------------------------------------------------------------------------

def _choose(split_below, torch_faster, C, B, T):
    if C in split_below and WN.split_in_range(B, T) and B * T < split_below[C]:
        return "split"
    return "torch" if C in torch_faster and (torch_faster[C] is None or B * T < torch_faster[C]) else "tiled"


def test_split_table_agrees_with_the_committed_measurements():
    """every single-layer case of profiles/wavenet_split_latency.json is routed by the shipped tables to whichever of the three
    sides was measured fastest there; without the file the table is empty"""
    if not os.path.exists(PROFILE):
        assert SHIPPED_SPLIT_BELOW == {}
        return
    with open(PROFILE) as f:
        doc = json.load(f)
    assert doc["H"] == H and doc["tile_split"] == TILE
    cases = [c for c in doc["cases"] if c["case"] == "layer"]
    assert {c["C"] for c in cases} == {384, 512}
    for C in (384, 512):
        assert {(c["B"], c["T"]) for c in cases if c["C"] == C} == {(1, 100), (1, 203), (1, 862), (4, 203), (48, 172)}
    assert set(SHIPPED_SPLIT_BELOW) <= {c["C"] for c in cases}
    for c in cases:
        assert c["frames"] == c["B"] * c["T"]
        times = {"torch": c["torch_ms"], "tiled": c["tiled_ms"], "split": c["split_ms"]}
        fastest = min(times, key=times.get)
        assert c["fastest"] == fastest
        assert _choose(SHIPPED_SPLIT_BELOW, SHIPPED_TORCH_FASTER, c["C"], c["B"], c["T"]) == fastest, (c["C"], c["B"], c["T"], times)
    for C in (384, 512):
        mine = sorted((c["frames"], c["fastest"]) for c in cases if c["C"] == C)
        assert mine[0][0] == 100
        if mine[0][1] != "split":                      # an entry only if the split form is the fastest at 1 x 100
            assert C not in SHIPPED_SPLIT_BELOW
            continue
        lost = [n for n, side in mine if side != "split"]
        assert SHIPPED_SPLIT_BELOW[C] == (lost[0] if lost else mine[-1][0] + 1)


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _stack_case(device, T=100, n=20):
    C = 384
    layers = [(O.seeded_weights(C, H, 370 + i), O.seeded_projection(C, 400 + i)) for i in range(n)]
    lt = [(_t(w, device), _t(p, device)) for w, p in layers]
    gen = torch.Generator().manual_seed(4)
    x, cond, s = torch.randn(1, C, T, generator=gen), torch.randn(1, H, T, generator=gen), torch.randn(1, C, generator=gen)
    return layers, lt, x.to(device), cond.to(device), s.to(device)


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical_and_allocates_only_its_buffers():
    """the 20-layer split stack at 1 x 100 is a chain of launches on the caller's stream: a capture of it has no parallel branches"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    layers, lt, x, cond, s = _stack_case(device)
    eager = WN.residual_stack(x, cond, s, lt, form="split")    # the warm call packs the tables, stacks the projections, sizes the workspace
    xn, cn, sn = x.cpu().numpy(), cond.cpu().numpy(), s.cpu().numpy()
    ref = O.stack(xn, cn, sn, layers)
    _check("split stack of 20 at 1 x 100", _np(eager), ref, _bars(_torch_stack(xn, cn, sn, layers), ref))
    tiled = WN.residual_stack(x, cond, s, lt, form="tiled")
    assert torch.equal(eager[0], tiled[0]) and torch.equal(eager[1], tiled[1])
    del tiled
    torch.cuda.synchronize()
    p0 = WN.PACKS["count"]
    nbytes = x.numel() * 4
    assert nbytes % 512 == 0
    d_bytes = -(-(20 * s.numel() * 4) // 512) * 512
    before = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    held = WN.residual_stack(x, cond, s, lt, form="split")
    assert torch.cuda.memory_allocated(device) - before == 2 * nbytes            # the two results stay
    assert torch.cuda.max_memory_allocated(device) - before <= 3 * nbytes + 2 * d_bytes   # + one hand-over buffer and d
    assert WN.PACKS["count"] == p0
    del held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, total = WN.residual_stack(x, cond, s, lt, form="split")
    for _ in range(2):
        y.fill_(NAN)
        total.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager[0]) and torch.equal(total, eager[1])


@pytest.mark.gpu
def test_gpu_non_default_stream_is_honoured():
    """x is produced on a side stream right before the call, without any synchronisation in between: only launches on that same
    stream are ordered behind it"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    _, lt, x, cond, s = _stack_case(device, T=203, n=1)
    d = s.clone()
    eager = WN.residual_layer(x, cond, d, lt[0][0], form="split")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    big = torch.randn(4096, 4096, device=device)
    xs = torch.zeros_like(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big @ big * 1e-2                     # keeps the side stream busy while the host runs ahead
        xs.copy_(x)
        y, sk = WN.residual_layer(xs, cond, d, lt[0][0], form="split")
    side.synchronize()
    assert torch.equal(y, eager[0]) and torch.equal(sk, eager[1])
