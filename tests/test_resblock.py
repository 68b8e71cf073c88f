"""The NSF-HiFiGAN residual blocks (ddsp_svc_amd.nsf_generator, csrc/resblock.h): the HIP kernel on the emulator and the GPU
against the float64 oracle, the zero-padded intermediate, the MRF epilogue, the dispatch, the C ABI and the reference hook.

The parity bar is relative to what float32 itself does on the same inputs: with e_torch = max|F.conv1d chain in float32 on the
CPU - oracle|, the kernel must stay within 4 e_torch + 1e-7 rms(oracle) (another summation order over up to 704 terms)."""
import os
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resblock_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import nsf_generator as NG  # noqa: E402

DILATIONS = [(1, 3, 5), (2, 1, 4)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resblock1.npz")


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def _torch_chain(x, weights, dilations):
    """the reference's op chain in float32 on the CPU"""
    x = torch.as_tensor(x)
    for (w1, b1, w2, b2), d in zip(weights, dilations):
        k = w1.shape[-1]
        xt = F.conv1d(F.leaky_relu(x, 0.1), torch.as_tensor(w1), torch.as_tensor(b1), dilation=d, padding=(k * d - d) // 2)
        xt = F.conv1d(F.leaky_relu(xt, 0.1), torch.as_tensor(w2), torch.as_tensor(b2), dilation=1, padding=(k - 1) // 2)
        x = xt + x
    return x.numpy()


def _bar(x, weights, dilations, ref):
    e_torch = float(np.abs(_torch_chain(x, weights, dilations).astype(np.float64) - ref).max())
    return 4.0 * e_torch + 1e-7 * _rms(ref), e_torch


def _tensors(weights, device):
    return [tuple(torch.from_numpy(a).to(device) for a in pair) for pair in weights]


# ---- the oracle against the reference's own output ------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 7, 11])
def test_oracle_matches_reference_fixture(k):
    g = np.load(GOLDEN)
    weights = [tuple(g["%s_%d_%d" % (n, k, p)] for n in ("w1", "b1", "w2", "b2")) for p in range(3)]
    want = O.block(g["x"], weights, (1, 3, 5))
    got = g["y_%d" % k].astype(np.float64)
    assert got.shape == (2, 16, 150)
    assert _rms(want) > 0.5                            # the conv terms are of the residual's size, not vanishing
    assert np.abs(got - want).max() <= 1e-5 * _rms(want)
    assert np.abs(_torch_chain(g["x"], weights, (1, 3, 5)) - g["y_%d" % k]).max() <= 1e-5 * _rms(want)


# ---- parity -------------------------------------------------------------------------------------------------------------------

def _parity_params():
    out = []
    for backend in BACKENDS:
        emu = backend == "emu"
        for C in (16, 32, 64):
            for k in (3, 7, 11):
                if emu and C == 64 and k != 11:        # the emulator runs an MFMA as a 64-fibre rendez-vous: C = 64 at k = 11 only
                    continue
                for dil in DILATIONS:
                    marks = [] if emu else [pytest.mark.gpu]
                    out.append(pytest.param(backend, C, k, dil, marks=marks,
                                            id="%s-C%d-k%d-d%s" % ("emu" if emu else "gpu", C, k, "".join(map(str, dil)))))
    return out


@pytest.mark.parametrize("dev,C,k,dil", _parity_params(), indirect=["dev"])
def test_parity(dev, C, k, dil):
    t = NG.tile(C, k)
    assert t == 128 - (k - 1)
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


# ---- edges: each conv pads its own input ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("C,k", [(16, 11), (32, 3)])
def test_intermediate_is_zero_outside_the_sequence(dev, C, k):
    t = NG.tile(C, k)
    dil = (1, 3, 5)
    weights = O.seeded_weights(C, k, 3, seed=7 * C + k, bias_std=1.0)
    wt = _tensors(weights, dev)
    rng = np.random.default_rng(k)
    for T in (1, t + 1):
        x = rng.standard_normal((2, C, T)).astype(np.float32)
        ref = O.block(x, weights, dil)
        bar, _ = _bar(x, weights, dil, ref)
        y = NG.resblock1(torch.from_numpy(x).to(dev), wt, dil).cpu().numpy().astype(np.float64)
        assert np.abs(y - ref).max() <= bar, (T, np.abs(y - ref).max(), bar)
        wrong = O.block(x, weights, dil, halo_from_padded_x=True)
        assert np.abs(wrong - ref).max() > 100 * bar, (T, np.abs(wrong - ref).max(), bar)   # the case can fail


# ---- the MRF epilogue -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_mrf_stage(dev):
    C, T = 16, NG.tile(16, 11) + 1
    blocks = [(O.seeded_weights(C, k, 3, seed=40 + k), dil) for k, dil in ((3, (1, 3, 5)), (7, (1, 3, 5)), (11, (2, 1, 4)))]
    x = np.random.default_rng(3).standard_normal((2, C, T)).astype(np.float32)
    ref = O.stage(x, blocks)
    xt = torch.from_numpy(x)
    chain = sum(torch.from_numpy(_torch_chain(x, w, d)) for w, d in blocks) / 3
    bar = 4.0 * float(np.abs(chain.numpy() - ref).max()) + 1e-7 * _rms(ref)
    y = NG.mrf_stage(xt.to(dev), [(_tensors(w, dev), d) for w, d in blocks])
    assert np.abs(y.cpu().numpy() - ref).max() <= bar


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_acc_aliased_to_the_output(dev):
    C, k, T, dil = 16, 7, 200, (1, 3, 5)
    weights = O.seeded_weights(C, k, 3, seed=5)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, C, T)).astype(np.float32)
    a = rng.standard_normal((2, C, T)).astype(np.float32)
    ref = a.astype(np.float64) + O.block(x, weights, dil)
    bar, _ = _bar(x, weights, dil, O.block(x, weights, dil))
    acc = torch.from_numpy(a.copy()).to(dev)
    y = NG.resblock1(torch.from_numpy(x).to(dev), _tensors(weights, dev), dil, acc=acc, out=acc)
    assert y is acc
    assert np.abs(y.cpu().numpy() - ref).max() <= bar + 1e-7 * np.abs(ref).max()            # + the rounding of the one more add
    sep = NG.resblock1(torch.from_numpy(x).to(dev), _tensors(weights, dev), dil, acc=torch.from_numpy(a).to(dev))
    assert torch.equal(sep, y)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_division_is_torch_div(dev):
    """zero weights and biases make a block the identity, exactly; the epilogue is then (acc + x) / 3 on a hand-made row"""
    C, k, T = 16, 3, 130
    zeros = [tuple(np.zeros(s, np.float32) for s in ((C, C, k), (C,), (C, C, k), (C,)))]
    row = np.arange(1, T + 1, dtype=np.float32) * np.float32(1.0009765625) + np.float32(0.3)
    x = np.tile(row, (1, C, 1)) * np.arange(1, C + 1, dtype=np.float32)[None, :, None]
    a = np.float32(0.7) * x[:, ::-1, ::-1].copy()
    want = torch.div(torch.from_numpy(a) + torch.from_numpy(x), 3)
    by_reciprocal = (torch.from_numpy(a) + torch.from_numpy(x)) * torch.tensor(1.0 / 3.0, dtype=torch.float32)
    assert not torch.equal(want, by_reciprocal)        # the row tells a division from a multiplication by 1 / 3
    y = NG.resblock1(torch.from_numpy(x).to(dev), _tensors(zeros, dev), (1,), acc=torch.from_numpy(a).to(dev), scale=3)
    assert torch.equal(y.cpu(), want)


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------

class _Block(torch.nn.Module):
    """a stand-in with the reference block's module tree: weight-normed ``convs1`` / ``convs2`` ModuleLists"""

    def __init__(self, C, k=3, dil=(1, 3, 5)):
        super().__init__()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wn = torch.nn.utils.weight_norm
            self.convs1 = torch.nn.ModuleList([wn(torch.nn.Conv1d(C, C, k, 1, dilation=d, padding=(k * d - d) // 2)) for d in dil])
            self.convs2 = torch.nn.ModuleList([wn(torch.nn.Conv1d(C, C, k, 1, dilation=1, padding=(k - 1) // 2)) for _ in dil])

    def remove_weight_norm(self):
        for c in list(self.convs1) + list(self.convs2):
            torch.nn.utils.remove_weight_norm(c)

    def chain(self, x):
        for c1, c2 in zip(self.convs1, self.convs2):
            x = c2(F.leaky_relu(c1(F.leaky_relu(x, 0.1)), 0.1)) + x
        return x

    def forward(self, x):
        return NG.resblock_forward(self, x)


def _counts():
    return NG.CALLS["hip"], NG.CALLS["reference"]


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_dispatch(dev):
    torch.manual_seed(0)
    x = torch.randn(2, 16, 50)
    blk = _Block(16)
    with torch.no_grad():
        h0, r0 = _counts()
        y = blk(x)                                     # weight-norm hooks present
        assert _counts() == (h0, r0 + 1) and torch.equal(y, blk.chain(x))
        blk.remove_weight_norm()
        y = blk(x)                                     # plain weights: the kernel
        assert _counts() == (h0 + 1, r0 + 1)
        assert (y - blk.chain(x)).abs().max() <= 1e-5
        big = _Block(128)
        big.remove_weight_norm()
        xb = torch.randn(1, 128, 20)
        yb = big(xb)                                   # 128 channels
        assert _counts() == (h0 + 1, r0 + 2) and torch.equal(yb, big.chain(xb))
        assert torch.equal(blk(x), y) and _counts() == (h0 + 2, r0 + 2)
        blk.double()
        assert blk(x.double()).dtype == torch.float64 and _counts() == (h0 + 2, r0 + 3)       # float64
        blk.float()
    xg = x.clone().requires_grad_(True)                # a gradient is needed: the reference's differentiable chain
    h1, r1 = _counts()
    yg = blk(xg)
    assert _counts() == (h1, r1 + 1) and yg.requires_grad
    yg.sum().backward()
    assert xg.grad is not None and blk.convs1[0].weight.grad is not None and torch.isfinite(xg.grad).all()
    with torch.no_grad():
        assert blk(xg) is not None and _counts() == (h1 + 1, r1 + 1)


def test_dispatch_keeps_host_tensors_on_the_reference():
    blk = _Block(16)
    blk.remove_weight_norm()
    x = torch.randn(1, 16, 30)
    with torch.no_grad():
        h0, r0 = _counts()
        assert torch.equal(blk(x), blk.chain(x)) and _counts() == (h0, r0 + 1)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_in_place_weight_update_invalidates_the_packed_cache(dev):
    torch.manual_seed(1)
    blk = _Block(16, k=7)
    blk.remove_weight_norm()
    x = torch.randn(1, 16, 40)
    with torch.no_grad():
        y0 = blk(x)
        assert (y0 - blk.chain(x)).abs().max() <= 1e-5
        assert torch.equal(blk(x), y0)                 # the cached table
        blk.convs2[1].weight.mul_(-2.0)
        blk.convs1[2].bias.add_(0.5)
        y1 = blk(x)
        assert (y1 - y0).abs().max() > 1e-2
        assert (y1 - blk.chain(x)).abs().max() <= 1e-5


class _Source(torch.nn.Module):
    """a seeded stand-in for the harmonic source (the reference's draws noise on every call)"""

    def forward(self, f0, upp):
        g = torch.Generator().manual_seed(5)
        return (0.1 * torch.randn(f0.shape[0], f0.shape[1] * upp, 1, generator=g)).to(f0)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_reference_generator_patched(dev):
    ref_root = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
    if not os.path.isdir(os.path.join(ref_root, "nsf_hifigan")):
        pytest.skip("reference checkout not present (only in the build container)")
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    for name in ["matplotlib", "matplotlib.pylab"]:
        sys.modules.setdefault(name, MagicMock())
    import nsf_hifigan.models as nm
    from nsf_hifigan.env import AttrDict
    h = AttrDict(num_mels=8, upsample_initial_channel=64, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], resblock="1",
                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, sampling_rate=44100)
    torch.manual_seed(2)
    gen = nm.Generator(h).eval()
    gen.m_source = _Source()
    with torch.no_grad():
        for p in gen.resblocks.parameters():           # the init's std 0.01 would leave only the residual
            p.mul_(8.0)
        mel, f0 = torch.randn(2, 8, 40), torch.full((2, 40), 220.0)
        before = gen(mel, f0)                          # weight norm still on: nothing to compare yet, the reference's own forward
        gen.remove_weight_norm()
        want = gen(mel, f0)
        assert (want - before).abs().max() <= 1e-5
        exact = gen.double()(mel.double(), f0.double()).numpy()
        gen.float().to(dev)
        try:
            NG.patch_reference_generator()
            h0, r0 = _counts()
            got = gen(mel.to(dev), f0.to(dev))
            assert _counts() == (h0 + 6, r0)           # two stages (32 and 16 channels) of three blocks
            for blk in gen.resblocks[:3]:              # one block through its own forward
                assert isinstance(blk, nm.ResBlock1) and blk(torch.randn(1, 32, 9).to(dev)).shape == (1, 32, 9)
            assert _counts() == (h0 + 9, r0)
        finally:
            NG.unpatch_reference_generator()
        assert "_reference_forward" not in nm.ResBlock1.__dict__ and "_reference_forward" not in nm.Generator.__dict__
    e_torch = float(np.abs(want.numpy() - exact).max())
    err = float(np.abs(got.cpu().numpy() - exact).max())
    print("generator: hip %.3e torch %.3e" % (err, e_torch))
    assert got.shape == want.shape == (2, 1, 160)
    assert err <= 4 * e_torch + 1e-7 * _rms(exact)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    import ctypes
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    assert [lib.ddsp_hip_resblock1_tile(16, k) for k in (3, 7, 11)] == [126, 122, 118]
    assert lib.ddsp_hip_resblock1_tile(128, 3) == 0 and lib.ddsp_hip_resblock1_tile(16, 5) == 0
    C, k, T = 16, 3, 20
    w, b = torch.randn(6, C, C, k) / (C * k) ** 0.5, 0.1 * torch.randn(6, C)
    need = lib.ddsp_hip_resblock1_pack_bytes(C, k, 3)
    assert need == 4 * 3 * (2 * C * C * k + 2 * C)
    assert lib.ddsp_hip_resblock1_pack_bytes(48, k, 3) == 0 and lib.ddsp_hip_resblock1_pack_bytes(C, 4, 3) == 0
    assert lib.ddsp_hip_resblock1_pack_bytes(C, k, 0) == 0 and lib.ddsp_hip_resblock1_pack_bytes(C, k, 9) == 0
    tab = torch.zeros(need // 4)
    assert lib.ddsp_hip_resblock1_pack(w.data_ptr(), b.data_ptr(), C, k, 3, tab.data_ptr(), need - 4) == -4
    assert lib.ddsp_hip_resblock1_pack(w.data_ptr(), b.data_ptr(), 24, k, 3, tab.data_ptr(), need) == -3
    assert lib.ddsp_hip_resblock1_pack(None, b.data_ptr(), C, k, 3, tab.data_ptr(), need) == -1
    assert lib.ddsp_hip_resblock1_pack(w.data_ptr(), b.data_ptr(), C, k, 3, tab.data_ptr(), need) == 0
    x = torch.randn(2, C, T)
    y = torch.full((2, C, T), 7.0)
    nws = lib.ddsp_hip_resblock1_workspace_bytes(2, C, T, 3)
    assert nws == 2 * 2 * C * T * 4 and lib.ddsp_hip_resblock1_workspace_bytes(2, C, T, 1) == 0
    ws = torch.zeros(nws // 4)
    dil = (ctypes.c_int * 3)(1, 3, 5)
    bad = {n: (ctypes.c_int * 3)(*v) for n, v in (("zero", (1, 0, 5)), ("neg", (-1, 3, 5)), ("huge", (1, 3, 100000)))}
    call = lambda **kw: lib.ddsp_hip_resblock1(*[kw.get(n, d) for n, d in (
        ("x", x.data_ptr()), ("y", y.data_ptr()), ("t", tab.data_ptr()), ("tb", need), ("B", 2), ("C", C), ("T", T), ("k", k),
        ("d", ctypes.addressof(dil)), ("p", 3), ("acc", None), ("s", 0.0), ("ws", ws.data_ptr()), ("wb", nws), ("st", None))])
    for kw, code in (({"C": 128}, -3), ({"C": 24}, -3), ({"k": 4}, -3), ({"k": 13}, -3), ({"T": 0}, -1), ({"T": -5}, -1),
                     ({"d": ctypes.addressof(bad["zero"])}, -1), ({"d": ctypes.addressof(bad["neg"])}, -1),
                     ({"d": ctypes.addressof(bad["huge"])}, -3), ({"d": None}, -1), ({"p": 0}, -1), ({"p": 9}, -3),
                     ({"B": -1}, -1), ({"x": None}, -1), ({"y": None}, -1), ({"t": None}, -1), ({"y": x.data_ptr()}, -1),
                     ({"tb": need - 4}, -4), ({"wb": nws - 4}, -4), ({"ws": None}, -4), ({"s": float("nan")}, -1)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all(), kw                    # refused before any launch
    assert call(B=0, x=None, y=None) == 0 and (y == 7.0).all()        # a no-op
    assert call() == 0
    weights = [(w[2 * p].numpy(), b[2 * p].numpy(), w[2 * p + 1].numpy(), b[2 * p + 1].numpy()) for p in range(3)]
    ref = O.block(x.numpy(), weights, (1, 3, 5))
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _gui_case(dev):
    C, k, T, dil = 16, 11, 512 * 203, (1, 3, 5)        # the sample-rate stage over the GUI's 2.35 s window
    wt = _tensors(O.seeded_weights(C, k, 3, seed=9), dev)
    x = torch.randn(1, C, T, generator=torch.Generator().manual_seed(4)).to(dev)
    return x, wt, dil


@pytest.mark.gpu
def test_gpu_call_allocates_only_the_output():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    x, wt, dil = _gui_case(dev)
    NG.resblock1(x, wt, dil)                           # packs the weights and sizes the hand-over buffer
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    y = NG.resblock1(x, wt, dil)
    after = torch.cuda.memory_allocated(dev)
    assert after - before == y.numel() * 4


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical():
    """every launch of a call goes to the caller's stream, one behind the other: a capture of it is a single chain"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    x, wt, dil = _gui_case(dev)
    eager = NG.resblock1(x, wt, dil)
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        NG.resblock1(x, wt, dil, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    ref = O.block(x[:, :, :600].cpu().numpy(), [tuple(t.cpu().numpy() for t in p) for p in wt], dil)
    assert np.abs(eager[:, :, :400].cpu().numpy() - ref[:, :, :400]).max() <= 1e-4   # columns the cut at 600 does not reach
