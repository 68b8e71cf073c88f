"""The channel-split form of the conformer conv module (ddsp_svc_amd.conformer with form="split", csrc/conformer_split.h): three
launches with a frame tile of 16, on the emulator and the GPU against the float64 oracle and, bit for bit, against the tiled form
(csrc/conformer_conv.h), whose sums it repeats in the same order; the traps of the tiled form's tests, the encoder, the range, the
C ABI, the encoder hook's three-way dispatch (split form, per-layer tiled form, torch) and the committed crossover table.

The parity bar is test_conformer.py's: 4 e_torch + 1e-7 rms(oracle), e_torch the error of the float32 torch op chain on the CPU on
the same inputs.  Every case prints its err / bar."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

from tests import conformer_oracle as O
from tests import conformer_standin as S
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_conformer import _bar, _t, _torch_chain

from ddsp_svc_amd import _ffi, conformer as CF  # noqa: E402

D = 256
T = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "conformer_split_latency.json")
NAN = float("nan")
# one partial tile, the tile edge, the first halo that crosses a tile, two and three tiles, the two real-time shapes (203 = 12
# tiles + 11 frames)
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 47, 100, 203)

SHIPPED_SPLIT_BELOW = dict(CF.CONV_SPLIT_BELOW)
SHIPPED_TORCH_FASTER = dict(CF.CONV_TORCH_FASTER)


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _check(tag, got, ref, bar):
    err = float(np.abs(got - ref).max())
    print("%s: err %.3e bar %.3e err / bar %.3f" % (tag, err, bar, err / bar))
    assert err <= bar, (tag, err, bar)


def _split(x, wt, device, **kw):
    return _np(CF.conv_module(torch.from_numpy(x).to(device), wt, form="split", **kw))


# ---- parity -------------------------------------------------------------------------------------------------------------------

_REFS = {}


def _parity_case(L, use_norm, add_input):
    """inputs, the oracle's result and the bar of one parity case, computed once for both backends"""
    key = (L, use_norm, add_input)
    if key not in _REFS:
        weights = O.seeded_weights(D, 10 + use_norm)
        norm = O.seeded_norm(D, 12) if use_norm else None
        x = np.random.default_rng(1000 + 4 * L + 2 * use_norm + add_input).standard_normal((2, L, D)).astype(np.float32)
        assert not np.array_equal(x[0], x[1])
        ref = O.net(x, weights, norm) + (x if add_input else 0.0)
        _REFS[key] = (x, weights, norm, ref, _bar(x, weights, ref, norm, add_input=add_input)[0])
    return _REFS[key]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("add_input", [False, True], ids=["net", "residual"])
@pytest.mark.parametrize("use_norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("L", LENGTHS)
def test_parity(dev, L, use_norm, add_input):
    assert CF.split_tile(D) == T
    x, weights, norm, ref, bar = _parity_case(L, use_norm, add_input)
    s0, h0 = CF.CALLS["split"], CF.CALLS["hip"]
    got = _split(x, _t(weights, dev), dev, norm=_t(norm, dev), add_input=add_input)
    assert (CF.CALLS["split"], CF.CALLS["hip"]) == (s0 + 1, h0 + 1)
    _check("split L %d norm %d add %d" % (L, use_norm, add_input), got, ref, bar)


# ---- the same bits as the tiled form ----------------------------------------------------------------------------------------------

def _both_forms(x, wt, nt, add_input, device):
    """(split, tiled): ``out`` and an explicit ``ws`` of exactly the split form's size hold NaN before the call"""
    B, L = x.shape[:2]
    got = []
    for form in ("split", "tiled"):
        xt = torch.from_numpy(x).to(device)
        kw = {}
        if form == "split":
            kw["ws"] = torch.full((_ffi.lib().ddsp_hip_conformer_conv_split_workspace_bytes(B, L, D) // 4,), NAN, device=device)
            assert kw["ws"].numel() == 4 * B * L * D
        y = CF.conv_module(xt, wt, norm=nt, add_input=add_input, out=torch.full_like(xt, NAN), form=form, **kw)
        assert torch.isfinite(y).all(), form
        got.append(y)
    return got


def _gate(x, weights, norm):
    """the pre-GLU gate rows W1[2 D:] ln(x) + b1[2 D:] in float64"""
    h = np.asarray(x, np.float64)
    if norm is not None:
        h = O.layer_norm(h, np.asarray(norm[0], np.float64), np.asarray(norm[1], np.float64), 1e-5)
    w1, b1 = np.asarray(weights[0], np.float64)[2 * D:, :, 0], np.asarray(weights[1], np.float64)[2 * D:]
    return h @ w1.T + b1


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B,L", [(1, L) for L in LENGTHS] + [(3, 33)])
@pytest.mark.parametrize("scale", (1.0, 100.0))
def test_same_bits_as_the_tiled_form(dev, scale, B, L):
    """scale 100: x (without LayerNorm) or gamma and beta (with it) a hundred times larger, so that the gate and the stencil
    saturate (expf overflows, the sigmoids are 0 or 1)"""
    weights, norm = O.seeded_weights(D, 20), O.seeded_norm(D, 21)
    x = np.random.default_rng(2000 + L + B).standard_normal((B, L, D)).astype(np.float32)
    big = tuple((np.float32(scale) * a).astype(np.float32) for a in norm)
    xs = (np.float32(scale) * x).astype(np.float32)
    wt = _t(weights, dev)
    for use_norm in (False, True):
        xin, nin = (x, big) if use_norm else (xs, None)
        if scale > 1.0:
            assert np.abs(_gate(xin, weights, nin)).max() > 100.0
        for add_input in (False, True):
            split, tiled = _both_forms(xin, wt, _t(nin, dev), add_input, dev)
            assert torch.equal(split, tiled), (use_norm, add_input)


# ---- the traps of the tiled form's tests ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_intermediate_is_zero_outside_the_sequence(dev):
    weights = O.seeded_weights(D, 20, bias_std=1.0)
    wt = _t(weights, dev)
    rng = np.random.default_rng(21)
    for L in (1, 17):
        x = rng.standard_normal((2, L, D)).astype(np.float32)
        ref = O.net(x, weights)
        bar, _ = _bar(x, weights, ref)
        _check("L %d" % L, _split(x, wt, dev), ref, bar)
        wrong = O.net(x, weights, halo_from_padded_x=True)
        assert np.abs(wrong - ref).max() > 100 * bar, (L, np.abs(wrong - ref).max(), bar)   # the case can fail


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_glu_halves_and_tap_orientation(dev):
    weights = O.seeded_weights(D, 30, asymmetric=True)
    x = np.random.default_rng(31).standard_normal((2, 40, D)).astype(np.float32)
    ref = O.net(x, weights)
    bar, _ = _bar(x, weights, ref)
    _check("asymmetric", _split(x, _t(weights, dev), dev), ref, bar)
    assert np.abs(O.net(x, weights, swap_glu=True) - ref).max() > 100 * bar
    assert np.abs(O.net(x, weights, flip_taps=True) - ref).max() > 100 * bar


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_layer_norm_edges(dev):
    """frame 0: all channels equal (variance 0: the result rests on eps); frame 1: mean 1e3 (a one-pass variance cancels in
    float32); a non-default eps"""
    weights, norm, eps = O.seeded_weights(D, 40), O.seeded_norm(D, 41), 0.1
    rng = np.random.default_rng(42)
    x = rng.standard_normal((2, 5, D)).astype(np.float32)
    x[:, 0, :] = np.float32(0.37)
    x[1, 0, :] = np.float32(-2.5)
    x[:, 1, :] = (1e3 + rng.standard_normal((2, D))).astype(np.float32)
    ref = O.net(x, weights, norm, eps)
    bar, _ = _bar(x, weights, ref, norm, eps)
    y = _split(x, _t(weights, dev), dev, norm=_t(norm, dev), eps=eps)
    assert np.isfinite(y).all()
    _check("layer norm edges", y, ref, bar)
    assert np.abs(O.net(x, weights, norm, 1e-5) - ref).max() > 100 * bar          # eps is not ignored
    tiled = CF.conv_module(torch.from_numpy(x).to(dev), _t(weights, dev), norm=_t(norm, dev), eps=eps)
    assert np.array_equal(_np(tiled), y)


# ---- the encoder and the packed cache -------------------------------------------------------------------------------------------

def _encoder_case(seed, device):
    layers = [(O.seeded_weights(D, seed + i), O.seeded_norm(D, seed + 10) if i == 1 else None, 1e-5) for i in range(3)]
    return layers, [(_t(w, device), _t(n, device), e) for w, n, e in layers]


def _encoder_ref_and_bar(x, layers):
    ref = O.encoder(x, layers)
    chain = x
    for w, n, e in layers:
        chain = _torch_chain(chain, w, n, e, add_input=True)
    return ref, 4.0 * float(np.abs(chain.astype(np.float64) - ref).max()) + 1e-7 * _rms(ref)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_encoder_and_packed_cache(dev):
    layers, lt = _encoder_case(50, dev)
    x = np.random.default_rng(51).standard_normal((2, 20, D)).astype(np.float32)
    xt = torch.from_numpy(x).to(dev)
    ref, bar = _encoder_ref_and_bar(x, layers)
    p0, s0, h0 = CF.PACKS["count"], CF.CALLS["split"], CF.CALLS["hip"]
    y = CF.encoder(xt, lt, form="split")
    assert CF.PACKS["count"] == p0 + 3 and (CF.CALLS["split"], CF.CALLS["hip"]) == (s0 + 3, h0 + 3)
    assert torch.equal(xt.cpu(), torch.from_numpy(x))                             # x is never written
    _check("split encoder", _np(y), ref, bar)
    tiled = CF.encoder(xt, lt, form="tiled")
    assert torch.equal(y, tiled) and torch.equal(y, CF.encoder(xt, lt))           # the default is the tiled form
    assert CF.PACKS["count"] == p0 + 3                                            # one table for both forms
    assert (CF.CALLS["split"], CF.CALLS["hip"]) == (s0 + 3, h0 + 9)
    out = torch.full_like(xt, NAN)
    assert CF.encoder(xt, lt, out=out, form="split") is out and torch.equal(out, y)
    # an in-place write bumps _version: one table is rebuilt once and both forms follow the new weight
    lt[2][0][4].mul_(-1.5)
    layers[2] = (tuple(a if i != 4 else (a * np.float32(-1.5)) for i, a in enumerate(layers[2][0])), None, 1e-5)
    y2 = CF.encoder(xt, lt, form="split")
    assert CF.PACKS["count"] == p0 + 4
    assert torch.equal(y2, CF.encoder(xt, lt, form="tiled")) and CF.PACKS["count"] == p0 + 4
    ref2, bar2 = _encoder_ref_and_bar(x, layers)
    assert np.abs(ref2 - ref).max() > 100 * bar2
    _check("split encoder, new weight", _np(y2), ref2, bar2)
    assert torch.equal(xt.cpu(), torch.from_numpy(x))
    for bad in (dict(form="flat"), dict(form=None), dict(form="split", out=xt)):
        with pytest.raises(ValueError):
            CF.encoder(xt, lt, **bad)
        with pytest.raises(ValueError):
            CF.conv_module(xt, lt[0][0], **bad)


# ---- range and refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_range_and_refusals(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    assert lib.ddsp_hip_conformer_conv_split_tile(D) == T == CF.split_tile(D)
    assert [lib.ddsp_hip_conformer_conv_split_tile(d) for d in (128, 512, 0, -256)] == [0] * 4
    ws_bytes = lib.ddsp_hip_conformer_conv_split_workspace_bytes
    assert ws_bytes(2, 6, D) == 4 * 2 * 6 * D * 4 and ws_bytes(0, 6, D) == 0
    assert ws_bytes(4096, 16, D) == 4 * 4096 * 16 * D * 4 and ws_bytes(1, 65536, D) == 4 * 65536 * D * 4
    assert [ws_bytes(*a) for a in ((-1, 6, D), (2, 0, D), (2, 6, 128), (2, 6, 512), (4097, 1, D), (4096, 17, D),
                                   (1, 65537, D))] == [0] * 7
    weights, norm = O.seeded_weights(D, 90), O.seeded_norm(D, 91)
    w = [torch.from_numpy(a) for a in weights + norm]
    need = lib.ddsp_hip_conformer_conv_pack_bytes(D, 1)
    plain = lib.ddsp_hip_conformer_conv_pack_bytes(D, 0)
    tab = torch.zeros(need // 4)
    assert lib.ddsp_hip_conformer_conv_pack(*[a.data_ptr() for a in w], D, tab.data_ptr(), need) == 0
    L = 6
    x = torch.randn(2, L, D, generator=torch.Generator().manual_seed(1))
    y = torch.full((2, L, D), 7.0)
    wsn = ws_bytes(2, L, D)
    ws = torch.zeros(wsn // 4)
    defaults = (("x", x.data_ptr()), ("y", y.data_ptr()), ("t", tab.data_ptr()), ("tb", need), ("ws", ws.data_ptr()), ("wb", wsn),
                ("B", 2), ("L", L), ("D", D), ("norm", 1), ("eps", 1e-5), ("add", 0), ("st", None))

    def call(**kw):
        return lib.ddsp_hip_conformer_conv_split(*[kw.get(n, v) for n, v in defaults])

    def tiled(**kw):
        return lib.ddsp_hip_conformer_conv(*[kw.get(n, v) for n, v in defaults if n not in ("ws", "wb")])

    # every refusal of the tiled entry (test_conformer.py::test_c_abi_refuses_bad_arguments), with the same code
    shared = (({"D": 128}, -3), ({"D": 512}, -3), ({"D": 0}, -3), ({"L": 0}, -1), ({"L": -1}, -1), ({"L": 2 ** 40 + 1}, -3),
              ({"y": x.data_ptr()}, -1), ({"tb": need - 4}, -4), ({"tb": plain}, -4), ({"x": None}, -1), ({"y": None}, -1),
              ({"t": None}, -1), ({"B": -1}, -1), ({"eps": float("nan")}, -1), ({"eps": float("inf")}, -1),
              ({"x": x.data_ptr() + 4}, -1), ({"y": y.data_ptr() + 4}, -1))
    for kw, code in shared:
        assert call(**kw) == code, kw
        assert tiled(**kw) == code, kw
        assert (y == 7.0).all() and (ws == 0.0).all(), kw                          # refused before any launch
    for kw, code in (({"ws": None}, -1), ({"wb": wsn - 4}, -4), ({"wb": 0}, -4), ({"ws": ws.data_ptr() + 2}, -1)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all() and (ws == 0.0).all(), kw
    # past the cap of 4096 tiles: a matter of shape, whatever the buffers hold
    huge = 4 * 4097 * 16 * D * 4
    for kw in ({"B": 4097, "L": 1}, {"B": 4097, "L": 16}, {"B": 4096, "L": 17}, {"B": 1, "L": 65537}, {"B": 2, "L": 32769}):
        assert call(wb=huge, **kw) == -3, kw
        assert (y == 7.0).all() and (ws == 0.0).all(), kw
    assert call(B=0, x=None, y=None, ws=None, wb=0) == 0 and (y == 7.0).all()      # a no-op
    assert call(norm=0, tb=plain) == 0                 # without the LayerNorm the shorter table is enough
    assert call() == 0
    ref = O.net(x.numpy(), weights, norm)
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    y2 = torch.full((2, L, D), 7.0)
    assert tiled(y=y2.data_ptr()) == 0 and torch.equal(y, y2)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_python_refuses_a_call_past_the_cap(dev):
    wt = _t(O.seeded_weights(D, 90), dev)
    assert CF.split_in_range(4096, 1) and CF.split_in_range(4096, 16) and CF.split_in_range(1, 65536)
    assert not CF.split_in_range(4097, 1) and not CF.split_in_range(4096, 17) and not CF.split_in_range(1, 65537)
    h0 = CF.CALLS["hip"]
    for B, L in ((4097, 1), (1, 65537)):
        x = torch.zeros(B, L, D)
        with pytest.raises(ValueError):
            CF.conv_module(x, wt, form="split")
        with pytest.raises(ValueError):
            CF.encoder(x, [(wt, None, 1e-5)], form="split")
    assert CF.CALLS["hip"] == h0
    with pytest.raises(RuntimeError, match="code -4"):     # a short workspace: DDSP_HIP_EWS from the entry point
        CF.conv_module(torch.zeros(1, 3, D), wt, form="split", ws=torch.zeros(4 * 3 * D - 1))


@pytest.mark.gpu
def test_at_the_cap():
    """B x tiles = 4096 at L = 1, utterance b = pool[b % 251] (251 is prime and 4096 mod 251 = 80: a wrong base or stride moves an
    utterance onto another pool entry), compared bitwise with the pool's own run, which the oracle checks; 4097 is refused"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    POOL, B, L = 251, 4096, 1
    weights, norm = O.seeded_weights(D, 80), O.seeded_norm(D, 82)
    wt, nt = _t(weights, device), _t(norm, device)
    xp = np.random.default_rng(81).standard_normal((POOL, L, D)).astype(np.float32)
    ref = O.net(xp, weights, norm) + xp
    xpool = torch.from_numpy(xp).to(device)
    ypool = CF.conv_module(xpool, wt, norm=nt, add_input=True, form="split")
    _check("pool", _np(ypool), ref, _bar(xp, weights, ref, norm, add_input=True)[0])
    flat = ref.reshape(POOL, -1)
    assert len({row.tobytes() for row in flat}) == POOL
    idx = torch.arange(B + 1, device=device) % POOL
    x = xpool[idx].contiguous()
    y = CF.conv_module(x[:B], wt, norm=nt, add_input=True, out=torch.full_like(x[:B], NAN), form="split")
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx[:B]])
    with pytest.raises(ValueError):
        CF.conv_module(x, wt, norm=nt, add_input=True, form="split")
    CF.release_workspace()


# ---- dispatch -------------------------------------------------------------------------------------------------------------------

def test_choose_form(monkeypatch):
    monkeypatch.setattr(CF, "CONV_TORCH_FASTER", {256: 27584})
    monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {})
    # an empty table: today's routing
    assert [CF.choose_form(D, B, L) for B, L in ((1, 100), (48, 172), (32, 862))] == [None, None, "tiled"]
    assert CF.choose_form(D, 1, 27583) is None and CF.choose_form(D, 1, 27584) == "tiled"
    monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: 4096})
    assert [CF.choose_form(D, B, L) for B, L in ((1, 100), (1, 203), (48, 172), (32, 862))] == ["split", "split", None, "tiled"]
    assert CF.choose_form(D, 1, 4095) == "split" and CF.choose_form(D, 1, 4096) is None
    assert CF.choose_form(512, 1, 100) == "tiled"          # a D without an entry in either table
    # over the cap of 4096 tiles never "split", whatever the table says
    monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: 10 ** 9})
    assert CF.choose_form(D, 4096, 1) == "split" and CF.choose_form(D, 4097, 1) is None
    assert CF.choose_form(D, 1, 65536) == "split" and CF.choose_form(D, 1, 65537) == "tiled"
    assert CF.choose_form(D, 4096, 16) == "split" and CF.choose_form(D, 4096, 17) == "tiled"
    monkeypatch.setattr(CF, "CONV_TORCH_FASTER", {})
    assert CF.choose_form(D, 4097, 1) == "tiled"


class Encoder(nn.Module):
    """``ConformerNaiveEncoder``'s one attribute, a ModuleList ``encoder_layers``; its ``forward`` is the package's dispatcher,
    as the reference's class has it after ``patch_reference_conformer()``"""

    def __init__(self, layers):
        super().__init__()
        self.encoder_layers = nn.ModuleList(layers)

    def forward(self, x, mask=None):
        return CF.encoder_forward(self, x, mask)


def _standin_encoder(seed, make=S.EncoderLayer, wrap=Encoder, attn_at=None, **kw):
    layers = []
    for i in range(3):
        layer = make(D, attn=S.ScaleAttn() if i == attn_at else None, use_norm=(i == 1), **kw)
        S.load(layer.conformer, O.seeded_weights(D, seed + i), O.seeded_norm(D, seed + 10) if i == 1 else None)
        layers.append(layer)
    return wrap(layers).eval()


def _specs(enc):
    return [CF._conv_spec(layer.conformer)[:3] for layer in enc.encoder_layers]


def _counts():
    return CF.CALLS["split"], CF.CALLS["hip"], CF.CALLS["reference"]


def _moved(c0):
    return tuple(a - b for a, b in zip(_counts(), c0))


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_encoder_hook_takes_the_split_form_below_the_bound(dev, monkeypatch):
    assert CF.CONV_TORCH_FASTER == {256: 27584}            # the shipped table stays in place throughout
    enc = _standin_encoder(300)
    L = 5
    x = torch.randn(1, L, D, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        want = x
        for layer in enc.encoder_layers:
            want = want + layer.conformer.net(want)
        tiled = CF.encoder(x, _specs(enc), form="tiled")
        # an empty table: 5 frames are torch's layer by layer, as today
        monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {})
        c0 = _counts()
        assert torch.equal(enc(x), want) and _moved(c0) == (0, 0, 3)
        monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: 4096})
        c0 = _counts()
        got = enc(x)
        assert _moved(c0) == (3, 3, 0)
        assert torch.equal(got, tiled)
        assert torch.equal(enc(x, None), got) and torch.equal(enc(x, mask=torch.ones(1, L, dtype=torch.bool)), got)
        assert _moved(c0) == (9, 9, 0)
        # a layer and a module called by themselves keep the two-way routing: torch at this size
        c0 = _counts()
        enc.encoder_layers[0](x)
        enc.encoder_layers[0].conformer(x)
        assert _moved(c0) == (0, 0, 2)
        # at and above the bound: back to per-layer dispatch
        for bound in (L, L - 1):
            monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: bound})
            c0 = _counts()
            assert torch.equal(enc(x), want) and _moved(c0) == (0, 0, 3)
        monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: L + 1})
        c0 = _counts()
        assert torch.equal(enc(x), got) and _moved(c0) == (3, 3, 0)
        # above the tiled form's crossover the layers take the tiled kernel one by one
        monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: L})
        monkeypatch.setattr(CF, "CONV_TORCH_FASTER", {256: L})
        c0 = _counts()
        assert torch.equal(enc(x), tiled) and _moved(c0) == (0, 3, 0)
    assert (got - want).abs().max() <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_encoder_hook_leaves_the_rest_to_the_reference_loop(dev, monkeypatch):
    monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: 4096})
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(9))

    def loop(enc, xin):
        for layer in enc.encoder_layers:
            xin = layer(xin, None)
        return xin

    with torch.no_grad():
        enc = _standin_encoder(320)
        c0 = _counts()
        ok = enc(x)
        assert _moved(c0) == (3, 3, 0)
        # one attention layer
        att = _standin_encoder(320, attn_at=1)
        c0 = _counts()
        y = att(x)
        assert _moved(c0) == (0, 0, 3) and torch.equal(y, loop(att, x)) and not torch.equal(y, ok)
        # a forward hook on a layer, a pre-hook on a conv module: the direct call would skip them
        seen = []
        hooked = _standin_encoder(320)
        handle = hooked.encoder_layers[1].register_forward_hook(lambda mod, inp, out: seen.append("layer"))
        c0 = _counts()
        assert torch.equal(hooked(x), loop(enc, x)) and _moved(c0) == (0, 0, 3 + 3) and seen == ["layer"]
        handle.remove()
        handle = hooked.encoder_layers[2].conformer.register_forward_pre_hook(lambda mod, inp: seen.append("conv"))
        c0 = _counts()
        hooked(x)
        assert _moved(c0) == (0, 0, 3) and seen == ["layer", "conv"]
        handle.remove()
        c0 = _counts()
        assert torch.equal(hooked(x), ok) and _moved(c0) == (3, 3, 0)
        # autocast
        with torch.autocast("cpu", dtype=torch.bfloat16):
            c0 = _counts()
            enc(x)
            assert _moved(c0) == (0, 0, 3)
        # an active dropout
        drop = _standin_encoder(320, dropout=0.1).train()
        c0 = _counts()
        drop(x)
        assert _moved(c0) == (0, 0, 3)
        c0 = _counts()
        assert torch.equal(drop.eval()(x), ok) and _moved(c0) == (3, 3, 0)
        # other tensors: float64, two dimensions, D = 128
        c0 = _counts()
        enc.double()(x.double())
        assert _moved(c0) == (0, 0, 3)
        enc.float()
        small = Encoder([S.EncoderLayer(128)]).eval()
        c0 = _counts()
        small(torch.randn(1, 5, 128))
        assert _moved(c0) == (0, 0, 1)
    # a needed gradient
    c0 = _counts()
    yg = enc(x.clone().requires_grad_(True))
    assert _moved(c0) == (0, 0, 3) and yg.requires_grad
    # weights that are inference tensors
    with torch.inference_mode():
        inf = _standin_encoder(320)
    with torch.no_grad():
        c0 = _counts()
        y = inf(x)
        assert _moved(c0) == (0, 0, 3)
    assert (y - ok).abs().max() <= 1e-5 * float(ok.abs().max())


def test_encoder_hook_keeps_host_tensors_on_the_reference(monkeypatch):
    monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: 4096})
    enc = _standin_encoder(340)
    x = torch.randn(1, 3, D)
    with torch.no_grad():
        c0 = _counts()
        got = enc(x)
        assert _moved(c0) == (0, 0, 3)
        want = x
        for layer in enc.encoder_layers:
            want = want + layer.conformer.net(want)
        assert torch.equal(got, want)


def _standin_module(name):
    """a module object with the reference's three class names, whose forwards are the classes' own op chains"""
    mod = types.ModuleType(name)

    class ConformerConvModule(S.ConvModule):
        def forward(self, x):
            return self.net(x)

    class CFNEncoderLayer(nn.Module):
        def __init__(self, dim, attn=None, **kw):
            super().__init__()
            self.conformer = ConformerConvModule(dim, **kw)
            self.norm = nn.LayerNorm(dim)
            self.attn = attn

        def forward(self, x, mask=None):
            if self.attn is not None:
                x = x + self.attn(self.norm(x), mask=mask)
            return x + self.conformer(x)

    class ConformerNaiveEncoder(nn.Module):
        def __init__(self, layers):
            super().__init__()
            self.encoder_layers = nn.ModuleList(layers)

        def forward(self, x, mask=None):
            for layer in self.encoder_layers:
                x = layer(x, mask)
            return x

    mod.ConformerConvModule, mod.CFNEncoderLayer, mod.ConformerNaiveEncoder = ConformerConvModule, CFNEncoderLayer, ConformerNaiveEncoder
    return mod


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_patch_round_trip_on_a_standin_module(dev, monkeypatch):
    M = _standin_module("reflow.model_conformer_naive")
    monkeypatch.setitem(sys.modules, "reflow.model_conformer_naive", M)
    monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: 4096})
    names = ("ConformerConvModule", "CFNEncoderLayer", "ConformerNaiveEncoder")
    originals = [getattr(M, n).forward for n in names]
    enc = _standin_encoder(360, make=M.CFNEncoderLayer, wrap=M.ConformerNaiveEncoder)
    x = torch.randn(2, 7, D, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        c0 = _counts()
        want = enc(x)
        assert _moved(c0) == (0, 0, 0)
        try:
            assert M in CF.patch_reference_conformer()
            patched = [getattr(M, n).forward for n in names]
            assert all(p is not o for p, o in zip(patched, originals))
            CF.patch_reference_conformer()             # idempotent
            assert [getattr(M, n).forward for n in names] == patched
            assert [getattr(M, n)._reference_forward for n in names] == originals
            got = enc(x)
            assert _moved(c0) == (3, 3, 0)
            monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {})
            assert torch.equal(enc(x), want) and _moved(c0) == (3, 3, 3)
        finally:
            CF.unpatch_reference_conformer()
        assert [getattr(M, n).forward for n in names] == originals
        assert not any("_reference_forward" in getattr(M, n).__dict__ for n in names)
        assert torch.equal(enc(x), want) and _moved(c0) == (3, 3, 3)
    assert (got - want).abs().max() <= 1e-5 * float(want.abs().max())


# ---- the real reference class -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_reference_encoder_through_the_patch(dev, monkeypatch):
    """Unit2Control's decoder with use_naive_v2: ConformerNaiveEncoder(3, 8, 256, False, True, ...)"""
    ref_root = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
    if not os.path.isdir(os.path.join(ref_root, "reflow")):
        pytest.skip("reference checkout not present (only in the build container)")
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    import reflow.model_conformer_naive as M
    enc_fwd = M.ConformerNaiveEncoder.forward
    monkeypatch.setattr(CF, "CONV_SPLIT_BELOW", {256: 4096})
    enc = M.ConformerNaiveEncoder(3, 8, D, False, True, 0, 0.1).eval()
    for i, layer in enumerate(enc.encoder_layers):     # the default initialisation would leave only the residual
        S.load(layer.conformer, O.seeded_weights(D, 100 + i))
    x = torch.randn(1, 100, D, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        want = enc(x)
        exact = enc.double()(x.double()).numpy()
        enc.float().to(dev)
        try:
            assert M in CF.patch_reference_conformer()
            assert M.ConformerNaiveEncoder.forward is not enc_fwd and M.ConformerNaiveEncoder._reference_forward is enc_fwd
            c0 = _counts()
            got = enc(x.to(dev))
            assert _moved(c0) == (3, 3, 0)
        finally:
            CF.unpatch_reference_conformer()
        assert M.ConformerNaiveEncoder.forward is enc_fwd and "_reference_forward" not in M.ConformerNaiveEncoder.__dict__
    e_torch = float(np.abs(want.numpy() - exact).max())
    _check("the reference's encoder through the patch", _np(got), exact, 4 * e_torch + 1e-7 * _rms(exact))


# ---- the committed table ----------------------------------------------------------------------------------------------------------

def _choose(split_below, torch_faster, d, B, L):
    if d in split_below and CF.split_in_range(B, L) and B * L < split_below[d]:
        return "split"
    return "torch" if d in torch_faster and (torch_faster[d] is None or B * L < torch_faster[d]) else "tiled"


def test_split_table_agrees_with_the_committed_measurements():
    """every plain-module case of profiles/conformer_split_latency.json is routed by the shipped tables to whichever of the three
    sides was measured fastest there; without the file the table is empty"""
    if not os.path.exists(PROFILE):
        assert SHIPPED_SPLIT_BELOW == {}
        return
    with open(PROFILE) as f:
        doc = json.load(f)
    assert doc["D"] == D and doc["tile_split"] == T
    cases = [c for c in doc["cases"] if c["case"] == "module"]
    assert {(c["B"], c["L"]) for c in cases} == {(1, 100), (1, 203), (1, 862), (4, 203), (48, 172)}
    assert set(SHIPPED_SPLIT_BELOW) <= {D}
    for c in doc["cases"]:
        assert c["split_equals_tiled"] is True, (c["case"], c["B"], c["L"])
    for c in cases:
        times = {"torch": c["torch_ms"], "tiled": c["tiled_ms"], "split": c["split_ms"]}
        fastest = min(times, key=times.get)
        assert c["fastest"] == fastest
        assert _choose(SHIPPED_SPLIT_BELOW, SHIPPED_TORCH_FASTER, D, c["B"], c["L"]) == fastest, (c["B"], c["L"], times)
    assert {int(k): v for k, v in doc["split_below"].items()} == SHIPPED_SPLIT_BELOW
    mine = sorted((c["frames"], c["fastest"]) for c in cases)
    if D not in SHIPPED_SPLIT_BELOW:
        assert mine[0][1] != "split"                   # no entry only if the split form is not the fastest at 1 x 100
        return
    assert mine[0][1] == "split"                       # an entry only if it is
    lost = [n for n, side in mine if side != "split"]
    assert SHIPPED_SPLIT_BELOW[D] == (lost[0] if lost else mine[-1][0] + 1)


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _gui_encoder(device, L=100):
    layers, lt = _encoder_case(370, device)
    x = torch.randn(1, L, D, generator=torch.Generator().manual_seed(4))
    return layers, lt, x.to(device)


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical_and_allocates_only_its_buffers():
    """the 3-layer split encoder at 1 x 100 is a chain of launches on the caller's stream: a capture of it has no parallel branches"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    layers, lt, x = _gui_encoder(device)
    eager = CF.encoder(x, lt, form="split")              # the warm call packs the tables and sizes the workspace
    ref, bar = _encoder_ref_and_bar(x.cpu().numpy(), layers)
    _check("split encoder of 3 at 1 x 100", _np(eager), ref, bar)
    assert torch.equal(eager, CF.encoder(x, lt, form="tiled"))
    torch.cuda.synchronize()
    p0 = CF.PACKS["count"]
    nbytes = -(-(x.numel() * 4) // 512) * 512
    before = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    held = CF.encoder(x, lt, form="split")
    assert torch.cuda.memory_allocated(device) - before == nbytes                # the result stays
    assert torch.cuda.max_memory_allocated(device) - before <= 2 * nbytes         # + one hand-over buffer
    assert CF.PACKS["count"] == p0
    del held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = CF.encoder(x, lt, form="split")
    for _ in range(2):
        y.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
    CF.release_workspace()


@pytest.mark.gpu
def test_gpu_non_default_stream_is_honoured():
    """x is produced on a side stream right before the call, without any synchronisation in between: only launches on that same
    stream are ordered behind it"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    _, lt, x = _gui_encoder(device, L=203)
    w, n, e = lt[1]
    eager = CF.conv_module(x, w, norm=n, eps=e, add_input=True, form="split")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    big = torch.randn(4096, 4096, device=device)
    xs = torch.zeros_like(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big @ big * 1e-2                     # keeps the side stream busy while the host runs ahead
        xs.copy_(x)
        y = CF.conv_module(xs, w, norm=n, eps=e, add_input=True, form="split")
    side.synchronize()
    assert torch.equal(y, eager)
    CF.release_workspace()
