"""The wide form of the NSF-HiFiGAN residual blocks (csrc/resblock_wide.h, 128 and 256 channels, one convolution per launch, the
input channels in chunks of 64 with one partial sum each): parity with the float64 oracle on the emulator and the GPU, the
zero-padded intermediate, the chunk and slice bookkeeping, the dilation limit, the MRF epilogue, the batch, the C ABI, the opt-in
route (``ROUTE_WIDE``) and the stand-in generator with it.

The bar is test_resblock.py's: with e_torch = max|F.conv1d chain in float32 on the CPU - oracle| on the same inputs, the kernel
must stay within 4 e_torch + 1e-7 rms(oracle)."""
import ctypes
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import pytest
import torch

from tests import generator_standin as S
from tests import resblock_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_resblock import _bar, _Block, _rms, _tensors, _torch_chain

from ddsp_svc_amd import _ffi
from ddsp_svc_amd import nsf_generator as NG  # noqa: E402

DILATIONS = [(1, 3, 5), (2, 1, 4)]
EMU_PARITY = ((128, 3), (128, 11), (256, 3))           # the emulator runs an MFMA as a 64-fibre rendez-vous
NAN = float("nan")


def _run(x, weights, dil, device, **kw):
    return NG.resblock1(torch.from_numpy(x).to(device), _tensors(weights, device), dil, **kw).cpu().numpy().astype(np.float64)


@pytest.fixture
def route_wide():
    """the route on and the wide shapes' measured ``TORCH_FASTER`` entries out of the way: what is held is the route, whatever
    the last measurement said"""
    kept = dict(NG.TORCH_FASTER)
    for key in kept:
        if key[0] in NG.WIDE_CHANNELS:
            del NG.TORCH_FASTER[key]
    NG.ROUTE_WIDE = True
    yield kept
    NG.ROUTE_WIDE = False
    NG.TORCH_FASTER.clear()
    NG.TORCH_FASTER.update(kept)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------

def _parity_params():
    out = []
    for backend in BACKENDS:
        emu = backend == "emu"
        for C in (128, 256):
            for k in (3, 7, 11):
                if emu and (C, k) not in EMU_PARITY:
                    continue
                for dil in DILATIONS:
                    out.append(pytest.param(backend, C, k, dil, marks=[] if emu else [pytest.mark.gpu],
                                            id="%s-C%d-k%d-d%s" % ("emu" if emu else "gpu", C, k, "".join(map(str, dil)))))
    return out


@pytest.mark.parametrize("dev,C,k,dil", _parity_params(), indirect=["dev"])
def test_parity(dev, C, k, dil):
    t = NG.wide_tile(C, k)
    assert t == 128 and NG.tile(C, k) == 0
    weights = O.seeded_weights(C, k, 3, seed=C * 100 + k)
    wt = _tensors(weights, dev)
    rng = np.random.default_rng(C + k + dil[0])
    worst = 0.0
    for T in (1, 7, t - 1, t, t + 1, 2 * t + 61):
        x = rng.standard_normal((2, C, T)).astype(np.float32)
        ref = O.block(x, weights, dil)
        bar, e_torch = _bar(x, weights, dil, ref)
        y = NG.resblock1(torch.from_numpy(x).to(dev), wt, dil).cpu().numpy().astype(np.float64)
        err = float(np.abs(y - ref).max())
        print("C %d k %d d %s T %d: hip %.3e torch %.3e bar %.3e ratio to torch %.2f" % (C, k, dil, T, err, e_torch, bar,
                                                                                         err / max(e_torch, 1e-30)))
        worst = max(worst, err / bar)
        assert err <= bar, (T, err, bar, e_torch)
    print("worst error / bar %.3f" % worst)


# ---- 2. each convolution pads its own input ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("C,k", [(128, 11), (256, 3)])
def test_intermediate_is_zero_outside_the_sequence(dev, C, k):
    t = NG.wide_tile(C, k)
    dil = (1, 3, 5)
    weights = O.seeded_weights(C, k, 3, seed=7 * C + k, bias_std=1.0)
    rng = np.random.default_rng(k)
    for T in (1, t + 1):
        x = rng.standard_normal((2, C, T)).astype(np.float32)
        ref = O.block(x, weights, dil)
        bar, _ = _bar(x, weights, dil, ref)
        err = float(np.abs(_run(x, weights, dil, dev) - ref).max())
        print("C %d k %d T %d: error / bar %.3f" % (C, k, T, err / bar))
        assert err <= bar, (T, err, bar)
        wrong = O.block(x, weights, dil, halo_from_padded_x=True)
        assert np.abs(wrong - ref).max() > 100 * bar, (T, np.abs(wrong - ref).max(), bar)   # the case can fail


# ---- 3. chunks and slices -------------------------------------------------------------------------------------------------------------

def _masked(C, k, rows, cols, rng):
    w = np.zeros((C, C, k), np.float32)
    w[64 * rows:64 * rows + 64, 64 * cols:64 * cols + 64] = rng.standard_normal((64, 64, k)) / np.sqrt(64 * k)
    return w


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_chunks_and_slices(dev):
    """One pair at C = 256, k = 3 without biases.  Conv 1 has weights only from input chunk c to output slice s, conv 2 only from
    chunk s (where conv 1 put its result) to slice c: over the sixteen (c, s) each convolution meets every (chunk, slice).  What
    the pair adds to its residual x is then non-zero in the rows of slice c and nowhere else: outside them y is x to the bit."""
    C, k, T, dil = 256, 3, 9, (2,)
    rng = np.random.default_rng(33)
    x = rng.standard_normal((2, C, T)).astype(np.float32)
    zero = np.zeros(C, np.float32)
    for c in range(4):
        for s in range(4):
            weights = [(_masked(C, k, s, c, rng), zero, _masked(C, k, c, s, rng), zero)]
            ref = O.block(x, weights, dil)
            bar, _ = _bar(x, weights, dil, ref)
            y = _run(x, weights, dil, dev)
            inside = np.zeros(C, bool)
            inside[64 * c:64 * c + 64] = True
            assert np.array_equal(y[:, ~inside], x[:, ~inside].astype(np.float64)), (c, s)
            assert np.abs(ref[:, inside] - x[:, inside]).max(axis=(0, 2)).min() > 1e-2, (c, s)      # every row of the slice moves
            assert np.abs(y - ref).max() <= bar, (c, s, np.abs(y - ref).max(), bar)


# ---- 4. the dilation limit ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_dilation_limit(dev):
    C, k = 128, 11
    t = NG.wide_tile(C, k)
    limit = max(d for d in range(1, 200) if NG.wide_shape_ok(C, k, (d,)))
    assert limit == 11                                 # 64 rows of 128 + 10 d columns, padded to 16 mod 32, in 64 KB
    assert max(d for d in range(1, 200) if NG.wide_shape_ok(C, 7, (d,))) == 18
    assert max(d for d in range(1, 200) if NG.wide_shape_ok(C, 3, (d,))) == 56
    assert not NG.wide_shape_ok(C, k, (0,)) and not NG.wide_shape_ok(64, k, (1,)) and not NG.wide_shape_ok(C, 5, (1,))
    assert not NG.wide_shape_ok(C, k, ()) and not NG.wide_shape_ok(C, k, (1,) * 9)
    T = t + 1
    weights = O.seeded_weights(C, k, 1, seed=77)
    x = np.random.default_rng(78).standard_normal((2, C, T)).astype(np.float32)
    ref = O.block(x, weights, (limit,))
    bar, _ = _bar(x, weights, (limit,), ref)
    err = float(np.abs(_run(x, weights, (limit,), dev) - ref).max())
    print("d = %d: error / bar %.3f" % (limit, err / bar))
    assert err <= bar
    xt, wt = torch.from_numpy(x).to(dev), _tensors(weights, dev)
    y = torch.full_like(xt, 7.0)
    with pytest.raises(ValueError):
        NG.resblock1(xt, wt, (limit + 1,), out=y)
    lib = _ffi.lib()
    nb = lib.ddsp_hip_resblock1_wide_pack_bytes(C, k, 1)
    tab = torch.zeros(nb // 4, device=dev)
    nws = lib.ddsp_hip_resblock1_wide_workspace_bytes(2, C, T, 1)
    ws = torch.zeros(nws // 4, device=dev)
    for d, code in ((limit + 1, -3), (100000, -3)):
        dil = (ctypes.c_int * 1)(d)
        assert lib.ddsp_hip_resblock1_wide(xt.data_ptr(), y.data_ptr(), tab.data_ptr(), nb, 2, C, T, k, ctypes.addressof(dil), 1,
                                           None, 0.0, ws.data_ptr(), nws, None) == code
    assert (y == 7.0).all()


# ---- 5. the MRF epilogue -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_mrf_stage(dev):
    C = 128
    T = NG.wide_tile(C, 11) + 1
    blocks = [(O.seeded_weights(C, k, 3, seed=40 + k), dil) for k, dil in ((3, (1, 3, 5)), (7, (1, 3, 5)), (11, (2, 1, 4)))]
    x = np.random.default_rng(3).standard_normal((2, C, T)).astype(np.float32)
    ref = O.stage(x, blocks)
    undivided = sum(torch.from_numpy(_torch_chain(x, w, d)) for w, d in blocks)
    bar = 4.0 * float(np.abs((undivided / 3).numpy() - ref).max()) + 1e-7 * _rms(ref)
    xt = torch.from_numpy(x).to(dev)
    tb = [(_tensors(w, dev), d) for w, d in blocks]
    y = NG.mrf_stage(xt, tb)
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print("mrf stage: error / bar %.3f" % (err / bar))
    assert err <= bar
    xs = None                                          # the same sum without the division: acc aliased to out
    for w, d in tb:
        r = NG.resblock1(xt, w, d, acc=xs, out=xs)
        assert xs is None or r is xs
        xs = r
    # an IEEE division: on the host, where torch.div by a number is one (on the GPU it multiplies by the reciprocal)
    assert torch.equal(y.cpu(), torch.div(xs.cpu(), 3))
    sep = NG.resblock1(xt, *tb[2], acc=NG.resblock1(xt, *tb[1], acc=NG.resblock1(xt, *tb[0])), scale=3)
    assert torch.equal(sep, y)                         # acc apart from out: the same bits


# ---- 6. the batch ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_rows_do_not_depend_on_the_batch(dev):
    C, k, dil = 128, 3, (1, 3, 5)
    T = NG.wide_tile(C, k) + 1
    wt = _tensors(O.seeded_weights(C, k, 3, seed=61), dev)
    x = torch.from_numpy(np.random.default_rng(62).standard_normal((3, C, T)).astype(np.float32)).to(dev)
    together = NG.resblock1(x, wt, dil)
    for b in range(3):
        assert torch.equal(NG.resblock1(x[b:b + 1], wt, dil), together[b:b + 1]), b
        assert not torch.equal(together[b], together[(b + 1) % 3])


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_batch_split(dev, knobs):
    """BATCH_SPLIT 2 and 1 at B = 5: chunks 2, 2, 1; three pairs, so the intermediate and both hand-over buffers are used at a
    non-zero base, with ``acc`` and ``scale = 3``"""
    C, k, dil, B, T = 128, 3, (1, 3, 5), 5, 7
    weights = O.seeded_weights(C, k, 3, seed=63)
    rng = np.random.default_rng(64)
    x, acc = rng.standard_normal((B, C, T)).astype(np.float32), rng.standard_normal((B, C, T)).astype(np.float32)
    ref = (acc.astype(np.float64) + O.block(x, weights, dil)) / 3
    chain = torch.div(torch.from_numpy(acc) + torch.from_numpy(_torch_chain(x, weights, dil)), 3)
    bar = 4.0 * float(np.abs(chain.numpy().astype(np.float64) - ref).max()) + 1e-7 * _rms(ref)
    wt, xt, at = _tensors(weights, dev), torch.from_numpy(x).to(dev), torch.from_numpy(acc).to(dev)

    def run():
        y = torch.full_like(xt, NAN)
        assert NG.resblock1(xt, wt, dil, acc=at, scale=3, out=y) is y
        return y
    whole = run()
    err = float(np.abs(whole.cpu().numpy().astype(np.float64) - ref).max())
    print("batch split: error / bar %.3f" % (err / bar))
    assert err <= bar
    rows = whole.cpu().numpy().reshape(B, -1)
    assert all(not np.array_equal(rows[i], rows[j]) for i in range(B) for j in range(i + 1, B))
    for split in (2, 1):
        knobs("BATCH_SPLIT", split)
        assert torch.equal(run(), whole), split


# ---- 7. the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    assert lib.ddsp_hip_resblock1_tile(128, 3) == 0    # the narrow entries take and refuse what they did
    assert [lib.ddsp_hip_resblock1_wide_tile(C, k) for C in (128, 256) for k in (3, 7, 11)] == [128] * 6
    assert [lib.ddsp_hip_resblock1_wide_tile(C, k) for C, k in ((64, 3), (16, 3), (192, 3), (512, 3), (128, 5))] == [0] * 5
    C, k, T = 128, 3, 20
    w, b = torch.randn(6, C, C, k) / (C * k) ** 0.5, 0.1 * torch.randn(6, C)
    need = lib.ddsp_hip_resblock1_wide_pack_bytes(C, k, 3)
    assert need == 4 * 3 * (2 * C * C * k + 2 * C)
    assert lib.ddsp_hip_resblock1_wide_pack_bytes(64, k, 3) == 0 and lib.ddsp_hip_resblock1_wide_pack_bytes(C, 4, 3) == 0
    assert lib.ddsp_hip_resblock1_wide_pack_bytes(C, k, 0) == 0 and lib.ddsp_hip_resblock1_wide_pack_bytes(C, k, 9) == 0
    assert lib.ddsp_hip_resblock1_wide_pack_bytes(256, 11, 1) == 4 * (2 * 256 * 256 * 11 + 512)
    tab = torch.zeros(need // 4)
    assert lib.ddsp_hip_resblock1_wide_pack(w.data_ptr(), b.data_ptr(), C, k, 3, tab.data_ptr(), need - 4) == -4
    assert lib.ddsp_hip_resblock1_wide_pack(w.data_ptr(), b.data_ptr(), 64, k, 3, tab.data_ptr(), need) == -3
    assert lib.ddsp_hip_resblock1_wide_pack(None, b.data_ptr(), C, k, 3, tab.data_ptr(), need) == -1
    assert lib.ddsp_hip_resblock1_wide_pack(w.data_ptr(), b.data_ptr(), C, k, 3, tab.data_ptr(), need) == 0
    x = torch.randn(2, C, T)
    y = torch.full((2, C, T), 7.0)
    act = 2 * C * T * 4
    assert [lib.ddsp_hip_resblock1_wide_workspace_bytes(2, C, T, p) for p in (1, 2, 3, 8)] == [act, 2 * act, 3 * act, 3 * act]
    assert lib.ddsp_hip_resblock1_wide_workspace_bytes(2, 64, T, 3) == 0 and lib.ddsp_hip_resblock1_wide_workspace_bytes(2, C, T, 9) == 0
    nws = 3 * act
    ws = torch.zeros(nws // 4)
    dil = (ctypes.c_int * 3)(1, 3, 5)
    bad = {n: (ctypes.c_int * 3)(*v) for n, v in (("zero", (1, 0, 5)), ("neg", (-1, 3, 5)), ("huge", (1, 3, 100000)),
                                                   ("past", (1, 57, 5)))}
    call = lambda **kw: lib.ddsp_hip_resblock1_wide(*[kw.get(n, d) for n, d in (
        ("x", x.data_ptr()), ("y", y.data_ptr()), ("t", tab.data_ptr()), ("tb", need), ("B", 2), ("C", C), ("T", T), ("k", k),
        ("d", ctypes.addressof(dil)), ("p", 3), ("acc", None), ("s", 0.0), ("ws", ws.data_ptr()), ("wb", nws), ("st", None))])
    for kw, code in (({"C": 64}, -3), ({"C": 16}, -3), ({"C": 192}, -3), ({"C": 512}, -3), ({"k": 4}, -3), ({"k": 13}, -3),
                     ({"T": 0}, -1), ({"T": -5}, -1), ({"T": (1 << 40) + 1}, -3),
                     ({"d": ctypes.addressof(bad["zero"])}, -1), ({"d": ctypes.addressof(bad["neg"])}, -1),
                     ({"d": ctypes.addressof(bad["huge"])}, -3), ({"d": ctypes.addressof(bad["past"])}, -3), ({"d": None}, -1),
                     ({"p": 0}, -1), ({"p": 9}, -3), ({"B": -1}, -1), ({"x": None}, -1), ({"y": None}, -1), ({"t": None}, -1),
                     ({"y": x.data_ptr()}, -1), ({"acc": x.data_ptr()}, -1), ({"tb": need - 4}, -4), ({"wb": nws - 4}, -4),
                     ({"ws": None}, -4), ({"ws": None, "wb": 0}, -4), ({"s": float("nan")}, -1)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all(), kw                    # refused before any launch
    assert call(B=0, x=None, y=None) == 0 and (y == 7.0).all()        # a no-op
    assert call() == 0
    weights = [(w[2 * p].numpy(), b[2 * p].numpy(), w[2 * p + 1].numpy(), b[2 * p + 1].numpy()) for p in range(3)]
    ref = O.block(x.numpy(), weights, (1, 3, 5))
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


# ---- 8. dispatch -------------------------------------------------------------------------------------------------------------------------

def _counts():
    return NG.CALLS["hip"], NG.CALLS["reference"]


def _plain_block(C, k, device):
    blk = _Block(C, k)
    blk.remove_weight_norm()
    return blk.to(device)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_dispatch(dev, route_wide):
    torch.manual_seed(0)
    C, k = 128, 3
    x = torch.randn(2, C, 50).to(dev)
    blk = _plain_block(C, k, dev)
    with torch.no_grad():
        want = blk.chain(x)
        NG.ROUTE_WIDE = False
        h, r = _counts()
        close = lambda a, b: (a - b).abs().max() <= 1e-5                           # torch's GPU convolutions do not repeat their bits
        assert close(blk(x), want) and _counts() == (h, r + 1)                     # the default: the reference chain
        NG.ROUTE_WIDE = True
        y = blk(x)
        assert _counts() == (h + 1, r + 1) and (y - want).abs().max() <= 1e-4      # the kernel
        assert torch.equal(blk(x), y) and _counts() == (h + 2, r + 1)
        normed = _Block(C, k).to(dev)                  # weight norm present
        h, r = _counts()
        assert normed(x).shape == x.shape and _counts() == (h, r + 1)
        blk.double()
        assert blk(x.double()).dtype == torch.float64 and _counts() == (h, r + 2)  # float64
        blk.float()
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            assert blk(x) is not None and _counts() == (h, r + 3)                  # autocast
        NG.TORCH_FASTER[(C, k)] = 51
        try:
            assert blk(x) is not None and _counts() == (h, r + 4)                  # measured faster on torch below T = 51
            NG.TORCH_FASTER[(C, k)] = 50
            assert torch.equal(blk(x), y) and _counts() == (h + 1, r + 4)
            NG.TORCH_FASTER[(C, k)] = None
            assert blk(x) is not None and _counts() == (h + 1, r + 5)              # ... at every T
        finally:
            del NG.TORCH_FASTER[(C, k)]
        NG.TORCH_FASTER.update(route_wide)             # the entries the measurement put in: all at T = 50 are torch's
        assert all(key in NG.TORCH_FASTER for key in ((c, kk) for c in (128, 256) for kk in (3, 7, 11)))
        assert close(blk(x), want) and _counts() == (h + 1, r + 6)
        for key in [key for key in NG.TORCH_FASTER if key[0] in NG.WIDE_CHANNELS]:
            del NG.TORCH_FASTER[key]
        narrow = _plain_block(16, k, dev)              # the narrow route is the same with the flag on
        h, r = _counts()
        assert narrow(torch.randn(1, 16, 20).to(dev)) is not None and _counts() == (h + 1, r)
    xg = x.clone().requires_grad_(True)                # a gradient is needed
    h, r = _counts()
    assert blk(xg).requires_grad and _counts() == (h, r + 1)
    with torch.inference_mode():                       # an inference tensor runs on the kernel
        xi = x.clone()
        assert xi.is_inference() and torch.equal(blk(xi), y) and _counts() == (h + 1, r + 1)


def test_crossover_table_agrees_with_the_committed_measurements():
    """every block of profiles/resblock_wide_{latency,throughput}.json is routed to whichever side was measured faster"""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    blocks = []
    for mode in ("latency", "throughput"):
        with open(os.path.join(root, "profiles", "resblock_wide_%s.json" % mode)) as f:
            doc = json.load(f)
        assert doc["stage_set"] == "wide" and (doc["B"], doc["frames"]) == ((1, 203) if mode == "latency" else (32, 861))
        blocks += doc["blocks"]
    assert {(b["C"], b["T"]) for b in blocks} == {(256, 8 * 203), (128, 64 * 203), (256, 8 * 861), (128, 64 * 861)}
    assert len(blocks) == 12
    from ddsp_svc_amd._modules import torch_faster
    for b in blocks:
        assert torch_faster(NG.TORCH_FASTER, (b["C"], b["k"]), b["T"]) == (b["torch_over_hip"] < 1.0), (b, NG.TORCH_FASTER)
    assert not any(key[0] in NG.CHANNELS for key in NG.TORCH_FASTER)     # the narrow stages have no measurement yet


def test_dispatch_keeps_host_tensors_on_the_reference(route_wide):
    blk = _plain_block(128, 3, "cpu")
    x = torch.randn(1, 128, 30)
    with torch.no_grad():
        h, r = _counts()
        assert torch.equal(blk(x), blk.chain(x)) and _counts() == (h, r + 1)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_in_place_weight_update_packs_again(dev, route_wide):
    torch.manual_seed(1)
    blk = _plain_block(128, 3, dev)
    x = torch.randn(1, 128, 40)
    with torch.no_grad():
        h, r = _counts()
        y0 = blk(x)
        assert (y0 - blk.chain(x)).abs().max() <= 1e-4
        assert torch.equal(blk(x), y0)                 # the cached table
        blk.convs2[1].weight.mul_(-2.0)
        blk.convs1[2].bias.add_(0.5)
        y1 = blk(x)
        assert (y1 - y0).abs().max() > 1e-2
        assert (y1 - blk.chain(x)).abs().max() <= 1e-4
        assert _counts() == (h + 3, r)


def test_unpatch_leaves_the_flag_off():
    ref_root = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
    if not os.path.isdir(os.path.join(ref_root, "nsf_hifigan")):
        pytest.skip("reference checkout not present (only in the build container)")
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    for name in ["matplotlib", "matplotlib.pylab"]:
        sys.modules.setdefault(name, MagicMock())
    try:
        nm = NG.patch_reference_generator(wide=True)
        assert NG.ROUTE_WIDE is True and nm.ResBlock1.forward is NG.resblock_forward
        NG.patch_reference_generator()
        assert NG.ROUTE_WIDE is False                  # the default, and the last call's word holds
        NG.patch_reference_generator(wide=True)
    finally:
        NG.unpatch_reference_generator()
    assert NG.ROUTE_WIDE is False and nm.ResBlock1.forward is not NG.resblock_forward


# ---- 9. the chain ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_chain_with_the_wide_route(dev, route_wide):
    """topology "a" of the stand-in: its 128-channel stage joins the nine blocks that run on HIP anyway"""
    from tests import test_generator_chain as G
    c = G._case("a")
    gen, mel, f0 = G._forward("a", dev)
    before = G._counts()
    got = G._np64(NG.generator_forward(gen, mel, f0))
    assert G._delta(before) == (12, 0, 3, 1, 1, 0)
    exact, fixture = c["rec"]["out"], c["g"]["out"].astype(np.float64)
    e_torch, rms = float(np.abs(fixture - exact).max()), _rms(exact)
    err = float(np.abs(got - exact).max())
    print("chain a, wide: hip %.3e torch %.3e ratio to torch %.2f" % (err, e_torch, err / e_torch))
    assert got.shape == exact.shape and err <= 4.0 * e_torch + 1e-7 * rms, (err, e_torch)
    x32 = c["rec"]["seam_0"].astype(np.float32)        # stage 0 alone, on the float32 rounding of the oracle's input
    before = G._counts()
    stage = NG.stage_forward(gen.stage_blocks(0), torch.from_numpy(x32).to(dev))
    assert G._delta(before) == (3, 0, 0, 0, 0, 0)
    G._check_step("a stage 0, wide", stage, S.BO.stage(x32, c["w"]["blocks"][0]), c["cpu"].torch_stage(0, torch.from_numpy(x32)))
    NG.ROUTE_WIDE = False
    before = G._counts()
    NG.generator_forward(gen, mel, f0)
    assert G._delta(before) == G.EXPECTED["a"]


# ---- 10. GPU only ------------------------------------------------------------------------------------------------------------------------

def _gui_case(device):
    C, k, T, dil = 128, 11, 64 * 203, (1, 3, 5)        # the 128-channel stage over the GUI's 2.35 s window
    wt = _tensors(O.seeded_weights(C, k, 3, seed=9), device)
    x = torch.randn(1, C, T, generator=torch.Generator().manual_seed(4)).to(device)
    return x, wt, dil


@pytest.mark.gpu
def test_gpu_call_allocates_only_the_output():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    x, wt, dil = _gui_case(device)
    NG.resblock1(x, wt, dil)                           # packs the weights and sizes the workspace
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(device)
    y = NG.resblock1(x, wt, dil)
    after = torch.cuda.memory_allocated(device)
    # the caching allocator hands out a cached block whole when less than 1 MiB of it would be left over, and counts all of it:
    # the output is 6.3 MiB, the weight table 4.1 MiB, one activation of the workspace 6.3 MiB
    assert y.numel() * 4 <= after - before < y.numel() * 4 + (1 << 20)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    assert NG.resblock1(x, wt, dil, out=y) is y        # into a given output: nothing at all, not even for a while
    assert torch.cuda.memory_allocated(device) == before and torch.cuda.max_memory_allocated(device) == before


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical():
    """every launch of a call goes to the caller's stream, one behind the other: a capture of it is a single chain"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    x, wt, dil = _gui_case(device)
    x2 = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(device)
    eager, eager2 = NG.resblock1(x, wt, dil), NG.resblock1(x2, wt, dil)
    static, out = x.clone(), torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        NG.resblock1(static, wt, dil, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2) and not torch.equal(eager, eager2)
    ref = O.block(x[:, :, :300].cpu().numpy(), [tuple(t.cpu().numpy() for t in p) for p in wt], dil)
    assert np.abs(eager[:, :, :150].cpu().numpy() - ref[:, :, :150]).max() <= 1e-4   # columns the cut at 300 does not reach
