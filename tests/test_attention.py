"""The performer attention (ddsp_svc_amd.attention, csrc/performer_attention.h): the HIP kernels on the emulator and the GPU against
the float64 oracle, the key chunks, the padding of features and frames, strided operands, the flat grids, the C ABI, the dispatch
and the reference hook.

The parity bar is test_conformer.py's, relative to what float32 itself does on the same inputs: with e_torch = max|the torch op
chain in float32 on the CPU - oracle|, the kernel must stay within 4 e_torch + 1e-7 rms(oracle).  Every case prints its err / bar."""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_oracle as O
from tests import attention_standin as S
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import _ffi, attention as AT  # noqa: E402

DH, M, H = 64, 266, 8
TILE = 64                                              # AT.tile(), which the parity test asserts
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "performer_attention.npz")
NAN = float("nan")

SHIPPED_TORCH_FASTER = dict(AT.ATTN_TORCH_FASTER)


@pytest.fixture(autouse=True)
def _structural_dispatch(monkeypatch):
    """the dispatch tests decide from a module's structure at shapes of a few frames: the measured crossover table (whose own
    test reads SHIPPED_TORCH_FASTER) is empty while they run, as it is in tools/attention_bench.py"""
    monkeypatch.setattr(AT, "ATTN_TORCH_FASTER", {})


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def _tt(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _bar(q, k, v, proj, ref, normalize=False):
    """(bar, e_torch): the float32 torch op chain on the CPU against the oracle"""
    chain = S.torch_chain(*_tt(q, k, v, proj), normalize).numpy().astype(np.float64)
    assert np.isfinite(chain).all()
    e_torch = float(np.abs(chain - ref).max())
    return 4.0 * e_torch + 1e-7 * _rms(ref), e_torch


def _run(q, k, v, proj, device, **kw):
    tq, tk, tv, tp = (t.to(device) for t in _tt(q, k, v, proj))
    return AT.fast_attention(tq, tk, tv, tp, **kw).cpu().numpy().astype(np.float64)


def test_crossover_table_agrees_with_the_committed_measurements():
    """every fast_attention case of profiles/attention_{throughput,latency}.json is routed to whichever side was measured faster"""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = []
    for mode in ("throughput", "latency"):
        with open(os.path.join(root, "profiles", "attention_%s.json" % mode)) as f:
            doc = json.load(f)
        assert doc["d"] == DH and doc["m"] == M and doc["tile"] == 64
        cases += [c for c in doc["cases"] if c["case"] == "fast_attention"]
    assert {c["frames"] for c in cases} == {100, 203, 48 * 172, 32 * 862}
    for c in cases:
        to_torch = DH in SHIPPED_TORCH_FASTER and (SHIPPED_TORCH_FASTER[DH] is None or c["frames"] < SHIPPED_TORCH_FASTER[DH])
        assert to_torch == (c["torch_over_hip"] < 1.0), (c["case"], c["frames"], c["torch_over_hip"], SHIPPED_TORCH_FASTER)


# ---- 1. the oracle against the reference's own output ----------------------------------------------------------------------------

def test_oracle_matches_reference_fixture():
    g = np.load(GOLDEN)
    q, k, v, proj = g["fast_q"], g["fast_k"], g["fast_v"], g["fast_proj"]
    assert q.shape == (2, 3, 37, 16) and proj.shape == (44, 16)
    for tag, flag in (("fast_y", False), ("fast_y_norm", True)):
        want = O.fast_attention(q, k, v, proj, flag)
        err, bar = float(np.abs(g[tag] - want).max()), 1e-5 * _rms(want)
        print("%s: err / bar %.3f" % (tag, err / bar))
        assert err <= bar
    assert np.abs(g["fast_y"] - g["fast_y_norm"]).max() > 1e-2 * _rms(g["fast_y"])   # the flag matters
    w = tuple(g["self_w%d" % i] for i in range(8))
    want = O.self_attention(g["self_x"], w, g["self_proj"], heads=2)
    err, bar = float(np.abs(g["self_y"] - want).max()), 1e-5 * _rms(want)
    print("self_y: err / bar %.3f" % (err / bar))
    assert g["self_y"].shape == (2, 37, 32) and err <= bar


# ---- 2. parity --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("scale", [0.5, 1.0, 4.0], ids=["0.5sigma", "1sigma", "4sigma"])
@pytest.mark.parametrize("N", [1, 7, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 17])
def test_parity(dev, N, scale, normalize):
    """at 4 sigma and N = 1, 7 the ``+ 1e-4`` of the query map and the ``+ 1e-8`` of the denominator decide the result (rms(out)
    far below 1)"""
    assert AT.tile() == TILE
    proj = O.seeded_projection(DH, M, 1)
    q, k, v = O.seeded_qkv(2, H, N, DH, seed=100 + N, scale=scale)
    ref = O.fast_attention(q, k, v, proj, normalize)
    flat = ref.reshape(2 * H, -1)
    assert len({row.tobytes() for row in flat}) == 2 * H                          # every (b, h) has its own data
    bar, e_torch = _bar(q, k, v, proj, ref, normalize)
    y = _run(q, k, v, proj, dev, normalize=normalize)
    assert np.isfinite(y).all()
    err = float(np.abs(y - ref).max())
    print("scale %.1f norm %d N %d: rms %.3e hip %.3e torch %.3e bar %.3e err / bar %.3f"
          % (scale, normalize, N, _rms(ref), err, e_torch, bar, err / bar))
    assert err <= bar, (N, err, bar, e_torch)


def test_small_constants_decide_the_result_at_four_sigma():
    """what the 4 sigma cases of the parity test are for: without ``+ 1e-4`` in the query map the oracle's result is another one"""
    proj = O.seeded_projection(DH, M, 1)
    q, k, v = O.seeded_qkv(2, H, 7, DH, seed=107, scale=4.0)
    ref = O.fast_attention(q, k, v, proj)
    assert _rms(ref) < 1e-2 * _rms(v)
    qp, kp = O.feature_map(q, proj, True) - M ** -0.5 * 1e-4, O.feature_map(k, proj, False)
    plain = (qp @ (np.swapaxes(kp, -1, -2) @ v)) / ((qp * kp.sum(-2)[..., None, :]).sum(-1, keepdims=True) + 1e-8)
    assert np.abs(plain - ref).max() > 0.1 * _rms(ref)


# ---- 3. key chunks ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_key_chunks(dev):
    t = AT.tile()
    N = 2 * t + 17
    proj = O.seeded_projection(DH, M, 2)
    q, k, v = O.seeded_qkv(1, 3, N, DH, seed=3)
    ref = O.fast_attention(q, k, v, proj)
    bar, _ = _bar(q, k, v, proj, ref)
    tq, tk, tv, tp = (a.to(dev) for a in _tt(q, k, v, proj))
    got = {}
    for chunks in (1, 2, 3, 50):
        y = AT.fast_attention(tq, tk, tv, tp, chunks=chunks)
        again = AT.fast_attention(tq, tk, tv, tp, chunks=chunks)
        assert torch.equal(y, again), chunks                                       # reproducible: no atomics
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print("chunks %d: err / bar %.3f" % (chunks, err / bar))
        assert err <= bar, chunks
        got[chunks] = y
    assert torch.equal(got[50], got[3])                                            # clamped to ceil(N / tile) = 3
    assert not torch.equal(got[1], got[2])                                         # another summation order: the chunks are real
    lib = _ffi.lib()
    assert lib.ddsp_hip_performer_workspace_bytes(1, 3, N, 50) == lib.ddsp_hip_performer_workspace_bytes(1, 3, N, 3)
    assert AT.default_chunks(1, H, 862) == 14 and AT.default_chunks(32, H, 862) == 1 and AT.default_chunks(1, 1, 64) == 1
    assert AT.default_chunks(2, H, 2 * t + 17) == 3 and AT.default_chunks(4, H, 10 * t) == 8
    with pytest.raises(ValueError):
        AT.fast_attention(tq, tk, tv, tp, chunks=0)


# ---- 4. padding -------------------------------------------------------------------------------------------------------------------

def _raw_call(device, q, k, v, table, chunks=1, normalize=0):
    """the C entry on contiguous [B, H, N, 64] tensors with a table of the caller's"""
    lib = _ffi.lib()
    B, Hh, N, _ = q.shape
    out = torch.full((B, Hh, N, DH), NAN, device=device)
    ws = torch.empty(lib.ddsp_hip_performer_workspace_bytes(B, Hh, N, chunks) // 4, device=device)
    strides = (_ffi.c_long * 12)(*(list(q.stride()[:3]) * 4))
    _ffi.check(lib.ddsp_hip_performer_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), strides, table.data_ptr(),
                                                table.numel() * 4, ws.data_ptr(), ws.numel() * 4, B, Hh, N, DH, M, normalize, chunks,
                                                _ffi.stream_of(q)))
    return out


def _packed(proj):
    lib = _ffi.lib()
    nbytes = lib.ddsp_hip_performer_pack_bytes(DH, M)
    assert nbytes == 17 * 16 * 64 * 4
    host = torch.full((nbytes // 4,), NAN)
    assert lib.ddsp_hip_performer_pack(proj.data_ptr(), DH, M, host.data_ptr(), nbytes) == 0
    return host


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_padding_of_frames_and_features(dev):
    t = AT.tile()
    proj = O.seeded_projection(DH, M, 4)
    tp = torch.from_numpy(proj).to(dev)
    # frames past N reach nothing: views of longer tensors whose tail is huge against the shorter tensors themselves, bit for bit
    for N, extra in ((5, 30), (t + 3, 20)):
        q, k, v = _tt(*O.seeded_qkv(2, 2, N + extra, DH, seed=40 + N))
        v[:, :, N:] = 1e30
        k[:, :, N:] = 3.0
        q, k, v = q.to(dev), k.to(dev), v.to(dev)
        for normalize in (False, True):
            part = AT.fast_attention(q[:, :, :N], k[:, :, :N], v[:, :, :N], tp, normalize=normalize, chunks=2)
            short = AT.fast_attention(q[:, :, :N].contiguous(), k[:, :, :N].contiguous(), v[:, :, :N].contiguous(), tp,
                                      normalize=normalize, chunks=2)
            assert torch.isfinite(part).all() and torch.equal(part, short), (N, normalize)
    # a zero key is not a missing key: the oracle with a zero frame appended gives another result, so the mask is needed
    q, k, v = O.seeded_qkv(1, 1, 5, DH, seed=45)
    ref = O.fast_attention(q, k, v, proj)
    zk, zv = np.concatenate([k, np.zeros_like(k[:, :, :1])], 2), np.concatenate([v, np.zeros_like(v[:, :, :1])], 2)
    wrong = O.fast_attention(np.concatenate([q, q[:, :, :1]], 2), zk, zv, proj)[:, :, :5]
    bar, _ = _bar(q, k, v, proj, ref)
    assert np.abs(wrong - ref).max() > 100 * bar
    # the last real feature (row 265) is live
    big = proj.copy()
    big[M - 1] *= 3.0
    q, k, v = O.seeded_qkv(2, 2, 20, DH, seed=46)
    ref = O.fast_attention(q, k, v, big)
    bar, _ = _bar(q, k, v, big, ref)
    err = float(np.abs(_run(q, k, v, big, dev) - ref).max())
    print("row 265 scaled: err / bar %.3f" % (err / bar))
    assert err <= bar
    dead = big.copy()
    dead[M - 1] = 0.0
    assert np.abs(O.fast_attention(q, k, v, dead) - ref).max() > 100 * bar
    # the table's padded rows (features 266 .. 271: fragment 16, lanes with (l & 15) >= 10) are zero as packed, and reach nothing
    # even as NaN
    host = _packed(torch.from_numpy(proj))
    frag = host.view(17, 16, 64)
    pad = (torch.arange(64) & 15) >= 10
    assert torch.isfinite(host).all() and (frag[16][:, pad] == 0).all() and (frag[16][:, ~pad] != 0).all()
    dn = DH ** -0.25
    assert frag[3, 5, 37].item() == pytest.approx(dn * proj[16 * 3 + (37 & 15), 4 * 5 + (37 >> 4)], rel=1e-6)
    poisoned = host.clone()
    poisoned.view(17, 16, 64)[16][:, pad] = NAN
    tq, tk, tv = (a.to(dev) for a in _tt(q, k, v))
    for normalize in (0, 1):
        clean = _raw_call(dev, tq, tk, tv, host.to(dev), chunks=1, normalize=normalize)
        dirty = _raw_call(dev, tq, tk, tv, poisoned.to(dev), chunks=1, normalize=normalize)
        assert torch.isfinite(dirty).all() and torch.equal(clean, dirty)
    assert torch.equal(clean.cpu(), AT.fast_attention(tq, tk, tv, tp, normalize=True, chunks=1).cpu())


# ---- 5. strides -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_strided_operands_and_out(dev):
    """q, k, v as the three slices of one [B, N, 3 H 64] buffer, the result into a [B, N, H 64] buffer: no copy on either side"""
    B, N = 2, AT.tile() + 5
    proj = torch.from_numpy(O.seeded_projection(DH, M, 5)).to(dev)
    buf = torch.randn(B, N, 3 * H * DH, generator=torch.Generator().manual_seed(50)).to(dev)
    q, k, v = (buf[..., i * H * DH:(i + 1) * H * DH].view(B, N, H, DH).permute(0, 2, 1, 3) for i in range(3))
    assert not q.is_contiguous() and k.data_ptr() == buf.data_ptr() + 4 * H * DH
    assert all(AT._kernel_view(a) is a for a in (q, k, v))                         # read in place
    want = AT.fast_attention(q.contiguous(), k.contiguous(), v.contiguous(), proj)
    out = torch.full((B, N, H * DH), NAN, device=dev)
    got = AT.fast_attention(q, k, v, proj, out=out)
    assert got.shape == (B, H, N, DH) and got.data_ptr() == out.data_ptr()
    assert torch.equal(got, want)
    assert torch.equal(out, want.permute(0, 2, 1, 3).reshape(B, N, H * DH))
    plain = AT.fast_attention(q, k, v, proj)
    assert plain.permute(0, 2, 1, 3).is_contiguous() and torch.equal(plain, want)  # 'b h n d -> b n (h d)' is a view
    odd = torch.randn(B, H, N, DH + 1, generator=torch.Generator().manual_seed(51)).to(dev)[..., :DH]   # strides no multiple of 4
    assert AT._kernel_view(odd) is not odd
    assert torch.equal(AT.fast_attention(odd, k, v, proj), AT.fast_attention(odd.contiguous(), k, v, proj))
    with pytest.raises(ValueError):
        AT.fast_attention(q, k, v, proj, out=torch.empty(B, N, H * DH + 1, device=dev))
    with pytest.raises(ValueError):
        AT.fast_attention(q, k, v[:, :, :-1], proj)
    with pytest.raises(ValueError):
        AT.fast_attention(q[..., :32], k[..., :32], v[..., :32], proj[:, :32])


# ---- 6. the grid limit --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("B,heads", [(8193, 8), (65537, 1)], ids=["BH_65544", "B_65537"])
def test_past_the_grid_limit(B, heads):
    """B H past 65 535 at N = 1: both grids are flat in x.  The first, the last and two middle items against the oracle; every item
    differs from the next.  The key partials take 70.7 KB per (b, h): 4.6 GB, released afterwards."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    proj = O.seeded_projection(DH, M, 6)
    q, k, v = O.seeded_qkv(B, heads, 1, DH, seed=60)
    try:
        tq, tk, tv, tp = (a.to(device) for a in _tt(q, k, v, proj))
        y = AT.fast_attention(tq, tk, tv, tp)
        assert torch.isfinite(y).all()
        y = y.cpu().numpy()
    finally:
        AT.release_workspace()
        torch.cuda.empty_cache()
    pick = [0, B // 3, 65535 // heads, B - 1]          # (the third holds workgroup 65 535)
    ref = O.fast_attention(q[pick], k[pick], v[pick], proj)
    bar, _ = _bar(q[pick], k[pick], v[pick], proj, ref)
    err = float(np.abs(y[pick] - ref).max())
    print("B %d H %d: err / bar %.3f" % (B, heads, err / bar))
    assert err <= bar
    assert not (y[1:] == y[:-1]).all(axis=(1, 2, 3)).any()


# ---- 7. the C ABI -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    assert lib.ddsp_hip_performer_tile(DH, M) == 64
    assert [lib.ddsp_hip_performer_tile(d, m) for d, m in ((32, 110), (64, 256), (64, 0), (0, 266), (-64, 266))] == [0] * 5
    need = 17 * 16 * 64 * 4
    assert lib.ddsp_hip_performer_pack_bytes(DH, M) == need
    assert [lib.ddsp_hip_performer_pack_bytes(d, m) for d, m in ((32, 110), (64, 272), (0, 0))] == [0, 0, 0]
    proj = torch.from_numpy(O.seeded_projection(DH, M, 7))
    tab = torch.zeros(need // 4)
    pack = lambda p=proj.data_ptr(), d=DH, m=M, t=tab.data_ptr(), n=need: lib.ddsp_hip_performer_pack(p, d, m, t, n)
    assert pack(n=need - 4) == -4
    assert pack(d=32) == -3 and pack(m=265) == -3
    assert pack(p=None) == -1 and pack(t=None) == -1
    assert pack() == 0
    B, N = 2, 6
    part = (272 * 64 + 272) * 4
    assert lib.ddsp_hip_performer_workspace_bytes(B, H, N, 1) == B * H * part
    assert lib.ddsp_hip_performer_workspace_bytes(B, H, 200, 3) == B * H * 3 * part
    assert lib.ddsp_hip_performer_workspace_bytes(B, H, 200, 9) == B * H * 4 * part   # clamped to ceil(200 / 64)
    assert [lib.ddsp_hip_performer_workspace_bytes(*a) for a in ((-1, H, N, 1), (B, 0, N, 1), (B, H, 0, 1), (B, H, N, 0))] == [0] * 4
    assert lib.ddsp_hip_performer_workspace_bytes(0, H, N, 1) == 0
    assert [lib.ddsp_hip_performer_chunks(*a) for a in ((-1, H, N), (B, 0, N), (B, H, 0))] == [0, 0, 0]
    q, k, v = _tt(*O.seeded_qkv(B, H, N, DH, seed=70))
    y = torch.full((B, H, N, DH), 7.0)
    ws = torch.zeros(B * H * part // 4)
    st = (_ffi.c_long * 12)(*(list(q.stride()[:3]) * 4))
    bad = lambda i, val: (_ffi.c_long * 12)(*[val if j == i else s for j, s in enumerate(st)])
    call = lambda **kw: lib.ddsp_hip_performer_attention(*[kw.get(n, d) for n, d in (
        ("q", q.data_ptr()), ("k", k.data_ptr()), ("v", v.data_ptr()), ("y", y.data_ptr()), ("st", st), ("t", tab.data_ptr()),
        ("tb", need), ("ws", ws.data_ptr()), ("wb", ws.numel() * 4), ("B", B), ("H", H), ("N", N), ("d", DH), ("m", M), ("norm", 0),
        ("chunks", 1), ("stream", None))])
    for kw, code in (({"d": 32}, -3), ({"m": 265}, -3), ({"d": 0}, -3), ({"N": 0}, -1), ({"N": -1}, -1), ({"N": 2 ** 30 + 1}, -3),
                     ({"B": 2 ** 31, "N": 64}, -3), ({"H": 0}, -1), ({"B": -1}, -1), ({"chunks": 0}, -1), ({"chunks": -2}, -1),
                     ({"q": None}, -1), ({"k": None}, -1), ({"v": None}, -1), ({"y": None}, -1), ({"st": None}, -1),
                     ({"t": None}, -1), ({"ws": None}, -1), ({"y": q.data_ptr()}, -1), ({"y": v.data_ptr()}, -1),
                     ({"q": q.data_ptr() + 4}, -1), ({"y": y.data_ptr() + 8}, -1), ({"st": bad(2, 66)}, -1),
                     ({"st": bad(9, -64)}, -1), ({"tb": need - 4}, -4), ({"wb": B * H * part - 4}, -4),
                     ({"N": 65, "chunks": 2}, -4)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all(), kw                    # refused before any launch
    assert call(B=0, q=None, k=None, v=None, y=None, ws=None, st=None, t=None) == 0 and (y == 7.0).all()   # a no-op
    assert call() == 0
    ref = O.fast_attention(q.numpy(), k.numpy(), v.numpy(), proj.numpy())
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    assert call(chunks=5) == 0                         # clamped to one tile: the workspace of one chunk is enough
    assert call(norm=1) == 0
    ref = O.fast_attention(q.numpy(), k.numpy(), v.numpy(), proj.numpy(), True)
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


# ---- 8. dispatch --------------------------------------------------------------------------------------------------------------------

def _counts():
    return AT.CALLS["hip"], AT.CALLS["reference"]


def _close(y, want):
    return float((y - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_dispatch(dev, monkeypatch):
    D, N = 256, 5
    torch.manual_seed(0)
    x = torch.randn(1, N, D)
    q, k, v = (torch.randn(1, H, N, DH) for _ in range(3))
    with torch.no_grad():
        fa = S.FastAttention()
        assert tuple(fa.projection_matrix.shape) == (M, DH)
        h0, r0 = _counts()
        y = fa(q, k, v)
        assert _counts() == (h0 + 1, r0) and _close(y, fa._reference_forward(q, k, v))
        sa = S.SelfAttention(D)
        h0, r0 = _counts()
        y = sa(x)
        assert _counts() == (h0 + 1, r0) and y.shape == x.shape
        assert _close(y, sa._reference_forward(x))     # (its core call is a launch of its own)
        wide = S.SelfAttention(128)                    # any input width
        h0, r0 = _counts()
        assert wide(torch.randn(1, N, 128)).shape == (1, N, 128) and _counts() == (h0 + 1, r0)
        idle = S.SelfAttention(D, dropout=0.1).eval()  # an inactive dropout
        assert idle(x) is not None and _counts() == (h0 + 2, r0)

        def to_reference(m, args, kw=None, kernel_inside=False):
            """the module's own forward runs and its result comes back; ``kernel_inside``: its inner FastAttention is eligible"""
            kw = kw or {}
            h1, r1 = _counts()
            y = m(*args, **kw)
            h2, r2 = _counts()
            assert r2 >= r1 + 1 and h2 == h1 + (1 if kernel_inside else 0), (h1, r1, h2, r2)
            want = m._reference_forward(*args, **kw)
            assert (torch.equal(y, want) if not kernel_inside else _close(y, want))

        mask = torch.ones(1, N, dtype=torch.bool)
        mask[0, -2:] = False
        to_reference(sa, (x,), {"mask": mask}, kernel_inside=True)                 # a mask: v is filled, then the core
        to_reference(sa, (x,), {"context": torch.randn(1, 3, D)}, kernel_inside=False)   # cross-attention: N differs, the core's own chain
        to_reference(S.SelfAttention(D, local_heads=2), (x,), kernel_inside=True)   # local heads: the global six still run the kernel
        to_reference(S.SelfAttention(D, dim_head=32), (x,))                        # dim_head = 32
        hooked = S.SelfAttention(D)
        hooked.to_q.register_forward_hook(lambda mod, inp, out: None)
        to_reference(hooked, (x,), kernel_inside=True)                             # a hook on a Linear
        to_reference(S.SelfAttention(D).double(), (x.double(),))                   # float64
        for kw in ({"causal": True}, {"generalized_attention": True}, {"no_projection": True}, {"nb_features": 256},
                   {"dim_heads": 32}):
            m = S.FastAttention(**kw)
            d = m.dim_heads
            to_reference(m, (q[..., :d], k[..., :d], v[..., :d]))
        assert AT.fast_eligible(fa, q, k, None) is None                            # v = None is the reference's
        # the crossover table
        monkeypatch.setitem(AT.ATTN_TORCH_FASTER, DH, N + 1)
        to_reference(fa, (q, k, v))
        to_reference(sa, (x,))
        monkeypatch.setitem(AT.ATTN_TORCH_FASTER, DH, N)
        h1, r1 = _counts()
        fa(q, k, v)
        sa(x)
        assert _counts() == (h1 + 2, r1)
        monkeypatch.setitem(AT.ATTN_TORCH_FASTER, DH, None)
        to_reference(fa, (q, k, v))
        monkeypatch.delitem(AT.ATTN_TORCH_FASTER, DH)
    # an active dropout: the module's own forward (seeded, so that both draws agree); the core inside is still the kernel's
    tr = S.SelfAttention(D, dropout=0.1).train()
    with torch.no_grad():
        h1, r1 = _counts()
        torch.manual_seed(5)
        y = tr(x)
        torch.manual_seed(5)
        want = tr._reference_forward(x)
        assert _counts() == (h1 + 2, r1 + 1) and _close(y, want)     # want's own core call is the second launch
        assert S.SelfAttention(D, dropout=0.0).train()(x) is not None and _counts() == (h1 + 3, r1 + 1)   # p = 0 is inactive
    # a gradient is needed: the differentiable chain; the same module under no_grad: the kernel
    xg = x.clone().requires_grad_(True)
    h1, r1 = _counts()
    yg = sa(xg)
    assert _counts() == (h1, r1 + 2) and yg.requires_grad                          # the module and its core
    yg.sum().backward()
    assert xg.grad is not None and sa.to_q.weight.grad is not None
    with torch.no_grad():
        sa(xg)
        assert _counts() == (h1 + 1, r1 + 2)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_dispatch_reads_the_flag_and_repacks_after_a_redraw(dev, monkeypatch):
    torch.manual_seed(1)
    q, k, v = (torch.randn(1, H, 9, DH) for _ in range(3))
    fa = S.FastAttention(seed=3)
    with torch.no_grad():
        for flag in (False, True, False):
            monkeypatch.setattr(S, "FLAG_PCMER_NORM", flag)
            ref = O.fast_attention(q.numpy(), k.numpy(), v.numpy(), fa.projection_matrix.numpy(), flag)
            bar, _ = _bar(q.numpy(), k.numpy(), v.numpy(), fa.projection_matrix.numpy(), ref, flag)
            assert np.abs(fa(q, k, v).numpy() - ref).max() <= bar, flag
        other = O.fast_attention(q.numpy(), k.numpy(), v.numpy(), fa.projection_matrix.numpy(), True)
        assert np.abs(other - ref).max() > 100 * bar                               # the flag is not a no-op here
        p0 = AT.PACKS["count"]
        fa(q, k, v)
        assert AT.PACKS["count"] == p0                                             # cached
        fa.redraw_projection_matrix(seed=9)                                        # copy_ in place: _version moves
        y = fa(q, k, v)
        assert AT.PACKS["count"] == p0 + 1
        ref2 = O.fast_attention(q.numpy(), k.numpy(), v.numpy(), fa.projection_matrix.numpy())
        assert np.abs(ref2 - ref).max() > 100 * bar and np.abs(y.numpy() - ref2).max() <= _bar(
            q.numpy(), k.numpy(), v.numpy(), fa.projection_matrix.numpy(), ref2)[0]
        fa(q, k, v)
        assert AT.PACKS["count"] == p0 + 1


def test_dispatch_keeps_host_tensors_on_the_reference():
    sa = S.SelfAttention(256)
    x = torch.randn(1, 3, 256)
    with torch.no_grad():
        h0, r0 = _counts()
        assert torch.equal(sa(x), sa._reference_forward(x)) and _counts()[0] == h0 and _counts()[1] > r0


# ---- 9. self_attention ------------------------------------------------------------------------------------------------------------

def _torch_self(x, w, proj, heads, normalize):
    x, proj = torch.as_tensor(x), torch.as_tensor(proj)
    wq, bq, wk, bk, wv, bv, wo, bo = (torch.as_tensor(a) for a in w)
    B, N, _ = x.shape
    q, k, v = (F.linear(x, a, b).view(B, N, heads, -1).permute(0, 2, 1, 3) for a, b in ((wq, bq), (wk, bk), (wv, bv)))
    o = S.torch_chain(q, k, v, proj, normalize)
    return F.linear(o.permute(0, 2, 1, 3).reshape(B, N, -1), wo, bo).numpy()


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
def test_self_attention(dev, normalize):
    D = 256
    w = O.seeded_linear(D, H, DH, seed=80)
    proj = O.seeded_projection(DH, M, 81)
    wt = [torch.from_numpy(a).to(dev) for a in w]
    tp = torch.from_numpy(proj).to(dev)
    for N in (1, AT.tile() + 1):
        x = np.random.default_rng(82 + N).standard_normal((2, N, D)).astype(np.float32)
        ref = O.self_attention(x, w, proj, H, normalize)
        e_torch = float(np.abs(_torch_self(x, w, proj, H, normalize) - ref).max())
        bar = 4.0 * e_torch + 1e-7 * _rms(ref)
        p0 = AT.PACKS["count"]
        y = AT.self_attention(torch.from_numpy(x).to(dev), *wt, tp, heads=H, normalize=normalize)
        assert y.shape == (2, N, D)
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print("norm %d N %d: hip %.3e torch %.3e err / bar %.3f" % (normalize, N, err, e_torch, err / bar))
        assert err <= bar, (N, err, bar)
        AT.self_attention(torch.from_numpy(x).to(dev), *wt, tp, heads=H, normalize=normalize)
        assert AT.PACKS["count"] <= p0 + 2                                         # at most the projection and the concatenation, once
    p0 = AT.PACKS["count"]
    wt[0].mul_(-1.0)                                                               # an in-place write: concatenated again
    AT.self_attention(torch.from_numpy(x).to(dev), *wt, tp, heads=H, normalize=normalize)
    assert AT.PACKS["count"] == p0 + 1


# ---- 10. the reference hook ---------------------------------------------------------------------------------------------------------

def test_patch_and_unpatch_on_a_stand_in_module():
    mod = types.ModuleType("standin_pcmer")

    class FastAttention(torch.nn.Module):
        def forward(self, q, k, v):
            return q

    class SelfAttention(torch.nn.Module):
        def forward(self, x, context=None, mask=None, context_mask=None, **kw):
            return x

    mod.FastAttention, mod.SelfAttention = FastAttention, SelfAttention
    fast_fwd, self_fwd = FastAttention.forward, SelfAttention.forward
    try:
        assert AT.patch_reference_attention([mod]) == [mod]
        patched = FastAttention.forward
        assert patched is not fast_fwd and SelfAttention.forward is not self_fwd
        assert FastAttention._reference_forward is fast_fwd and SelfAttention._reference_forward is self_fwd
        AT.patch_reference_attention([mod])            # idempotent
        assert FastAttention.forward is patched and FastAttention._reference_forward is fast_fwd
        x = torch.randn(1, 2, 4)
        r0 = AT.CALLS["reference"]
        assert SelfAttention()(x, mask=None) is x and FastAttention()(x, x, x) is x   # nothing eligible: the originals run
        assert AT.CALLS["reference"] == r0 + 2
    finally:
        AT.unpatch_reference_attention([mod])
    assert FastAttention.forward is fast_fwd and SelfAttention.forward is self_fwd
    assert "_reference_forward" not in FastAttention.__dict__ and "_reference_forward" not in SelfAttention.__dict__
    AT.unpatch_reference_attention([mod])              # nothing parked: nothing happens
    assert FastAttention.forward is fast_fwd


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_reference_hook(dev, monkeypatch):
    ref_root = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
    if not os.path.isfile(os.path.join(ref_root, "ddsp", "pcmer.py")):
        pytest.skip("reference checkout not present (only in the build container)")
    for name in ("gin", "local_attention"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, MagicMock())
    if ref_root not in sys.path:
        monkeypatch.syspath_prepend(ref_root)
    import ddsp.pcmer as P
    fast_fwd, self_fwd = P.FastAttention.forward, P.SelfAttention.forward
    torch.manual_seed(3)
    enc = P.PCmer(3, H, 256, 64, 64, 0.1, 0.1).eval()
    x = torch.randn(1, 20, 256, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        want = enc(x)
        exact = enc.double()(x.double()).numpy()
        enc.float()
        try:
            assert AT.patch_reference_attention() == [P]
            assert P.SelfAttention.forward is not self_fwd and P.SelfAttention._reference_forward is self_fwd
            h0, r0 = _counts()
            got = enc(x)
            assert _counts() == (h0 + 3, r0)
            one = enc._layers[0].attn.fast_attention(*(torch.randn(1, H, 4, DH) for _ in range(3)))   # the core through its own forward
            assert one.shape == (1, H, 4, DH) and _counts() == (h0 + 4, r0)
        finally:
            AT.unpatch_reference_attention()
        assert P.FastAttention.forward is fast_fwd and P.SelfAttention.forward is self_fwd
        assert "_reference_forward" not in P.SelfAttention.__dict__
    e_torch = float(np.abs(want.numpy() - exact).max())
    err = float(np.abs(got.numpy() - exact).max())
    bar = 4 * e_torch + 1e-7 * _rms(exact)
    print("PCmer through the hook: hip %.3e torch %.3e err / bar %.3f" % (err, e_torch, err / bar))
    assert err <= bar


# ---- 12. GPU only -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical():
    """a call is two launches on the caller's stream, one behind the other: a capture of it has no parallel branches"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    proj = O.seeded_projection(DH, M, 90)
    q, k, v = O.seeded_qkv(1, H, 203, DH, seed=91)                                 # the GUI's 2.35 s window
    ref = O.fast_attention(q, k, v, proj)
    bar, _ = _bar(q, k, v, proj, ref)
    tq, tk, tv, tp = (a.to(device) for a in _tt(q, k, v, proj))
    eager = AT.fast_attention(tq, tk, tv, tp)                                       # the warm call packs the table
    torch.cuda.synchronize()
    assert np.abs(eager.cpu().numpy() - ref).max() <= bar
    out = torch.empty(1, 203, H * DH, device=device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        AT.fast_attention(tq, tk, tv, tp, out=out)
    for _ in range(2):
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(1, 203, H, DH).permute(0, 2, 1, 3), eager)
