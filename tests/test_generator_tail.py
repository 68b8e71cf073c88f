"""The NSF-HiFiGAN generator's upsampling seam and output head (ddsp_svc_amd.nsf_generator, csrc/generator_tail.h): the HIP
kernels on the emulator and the GPU against the float64 oracle, the wrong variants the cases can tell apart, the dispatch, the C
ABI and the reference hook.

The parity bar is the one of test_resblock.py: with e_torch = max|the float32 torch chain on the CPU - oracle| (here
F.conv_transpose1d + F.conv1d, and F.conv1d + torch.tanh), the kernel must stay within 4 e_torch + 1e-7 rms(oracle).  e_torch is
the maximum over all lengths of a parametrised case: at T = 1 a single case has too few elements to be a stable yardstick."""
import os
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import generator_tail_oracle as O
from tests import resblock_oracle as BO
from tests.backends import BACKENDS, dev  # noqa: F401

from ddsp_svc_amd import nsf_generator as NG  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generator_tail.npz")
SEAM_CASES = [(64, 2, 4), (32, 2, 2), (16, 2, 1), (16, 4, 2), (16, 8, 1)]          # (Cout, u, s): the stock three, then u = 4, 8
HEAD_CHANNELS = (16, 32, 64)


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def _t(arrays, device):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def _torch_seam(x, w, u, src, s):
    """the reference's op chain in float32 on the CPU"""
    wu, bu, wn, bn = [torch.as_tensor(a) for a in w]
    up = F.conv_transpose1d(F.leaky_relu(torch.as_tensor(x), 0.1), wu, bu, stride=u, padding=(2 * u - u) // 2)
    return (up + F.conv1d(torch.as_tensor(src), wn, bn, stride=s, padding=s // 2 if s > 1 else 0)).numpy()


def _torch_head(x, w, slope=0.01):
    return torch.tanh(F.conv1d(F.leaky_relu(torch.as_tensor(x), slope), torch.as_tensor(w[0]), torch.as_tensor(w[1]), padding=3)).numpy()


def _seam_inputs(rng, B, Cout, u, s, Tin):
    x = rng.standard_normal((B, 2 * Cout, Tin)).astype(np.float32)
    src = rng.standard_normal((B, 1, s * u * Tin)).astype(np.float32)
    return x, src


def _seam_run(dev, x, w, u, src, s):
    wt = _t(w, dev)
    y = NG.upsample_stage(torch.from_numpy(x).to(dev), wt[0], wt[1], u, torch.from_numpy(src).to(dev), wt[2], wt[3], s)
    return y.cpu().numpy().astype(np.float64)


def _head_run(dev, x, w, slope=0.01):
    wt = _t(w, dev)
    return NG.output_head(torch.from_numpy(x).to(dev), wt[0], wt[1], slope).cpu().numpy().astype(np.float64)


# ---- the oracle against the reference's own output ------------------------------------------------------------------------------

def test_oracle_matches_reference_fixture():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200000
    assert np.array_equal(O.lrelu(g["pre_out"].astype(np.float64)).astype(np.float32), g["up_in_0"])   # lrelu 0.1, to the bit
    for i, (Cout, s, Tin) in enumerate(((32, 2, 20), (16, 1, 40))):
        got = g["stage_in_%d" % i].astype(np.float64)
        assert got.shape == (2, Cout, 2 * Tin)
        up = O.conv_transpose(g["up_in_%d" % i], g["wu_%d" % i], g["bu_%d" % i], 2)
        nz = O.noise_conv(g["source"][:, 0], g["wn_%d" % i], g["bn_%d" % i], s)
        assert _rms(up) > 0.5 and _rms(nz) > 0.5       # both terms are of order one: neither hides behind the other
        assert np.abs(got - (up + nz)).max() <= 1e-5 * _rms(up + nz)
    want = O.head(g["post_in"], g["wp"], g["bp"], slope=1.0)     # post_in went through lrelu 0.01 already
    assert g["out"].shape == (2, 1, 80) and 0.3 < _rms(want) < 0.9                 # tanh neither linear nor saturated
    assert np.abs(g["out"] - want).max() <= 1e-5 * _rms(want)


def test_oracle_seam_is_the_torch_chain():
    """what the fixture cannot reach: u = 4 and 8, s = 4, the lrelu inside ``seam`` and ``head``, lengths 1 and 2"""
    rng = np.random.default_rng(1)
    for Cout, u, s in SEAM_CASES:
        w = O.seeded_seam_weights(Cout, u, s, seed=u + s)
        for Tin in (1, 2, 5):
            x, src = _seam_inputs(rng, 2, Cout, u, s, Tin)
            ref = O.seam(x, *w[:2], u, src, *w[2:], s)
            assert np.abs(_torch_seam(x, w, u, src, s) - ref).max() <= 1e-5 * _rms(ref)
    w = O.seeded_head_weights(16, seed=3)
    x = rng.standard_normal((2, 16, 9)).astype(np.float32)
    assert np.abs(_torch_head(x, w) - O.head(x, *w)).max() <= 1e-6


# ---- parity -------------------------------------------------------------------------------------------------------------------

def _backend_params(cases, ids):
    out = []
    for backend in BACKENDS:
        emu = backend == "emu"
        for case, name in zip(cases, ids):
            out.append(pytest.param(backend, case, marks=[] if emu else [pytest.mark.gpu], id="%s-%s" % ("emu" if emu else "gpu", name)))
    return out


# Cout = 64 has a single case, so the emulator (an MFMA is a 64-fibre rendez-vous there) runs 64 channels once
@pytest.mark.parametrize("dev,case", _backend_params(SEAM_CASES, ["C%d-u%d-s%d" % c for c in SEAM_CASES]), indirect=["dev"])
def test_seam_parity(dev, case):
    Cout, u, s = case
    tq = NG.seam_tile(Cout, u)
    assert tq == (64 if (Cout, u) == (64, 8) else 128)
    w = O.seeded_seam_weights(Cout, u, s, seed=100 * Cout + 10 * u + s)
    rng = np.random.default_rng(Cout + u + s)
    runs = []
    for Tin in (1, 2, tq - 1, tq, tq + 1, 2 * tq + 5):
        x, src = _seam_inputs(rng, 2, Cout, u, s, Tin)
        ref = O.seam(x, *w[:2], u, src, *w[2:], s)
        e_t = float(np.abs(_torch_seam(x, w, u, src, s) - ref).max())
        y = _seam_run(dev, x, w, u, src, s)
        assert y.shape == ref.shape == (2, Cout, u * Tin)
        runs.append((Tin, float(np.abs(y - ref).max()), e_t, _rms(ref)))
    e_torch = max(r[2] for r in runs)
    for Tin, err, e_t, rms in runs:
        bar = 4.0 * e_torch + 1e-7 * rms
        print("Cout %d u %d s %d Tin %d: hip %.3e torch %.3e (case %.3e) bar %.3e ratio to torch %.2f" % (
            Cout, u, s, Tin, err, e_t, e_torch, bar, err / e_torch))
    for Tin, err, e_t, rms in runs:
        assert err <= 4.0 * e_torch + 1e-7 * rms, (Tin, err, e_torch)


@pytest.mark.parametrize("dev,C", _backend_params(HEAD_CHANNELS, ["C%d" % c for c in HEAD_CHANNELS]), indirect=["dev"])
def test_head_parity(dev, C):
    tile = NG.head_tile(C)
    assert tile == 1024
    w = O.seeded_head_weights(C, seed=C)
    rng = np.random.default_rng(C)
    runs = []
    for T in (1, 3, 4, tile - 1, tile, tile + 1, 2 * tile + 9):
        x = rng.standard_normal((2, C, T)).astype(np.float32)
        ref = O.head(x, *w)
        e_t = float(np.abs(_torch_head(x, w) - ref).max())
        y = _head_run(dev, x, w)
        assert y.shape == ref.shape == (2, 1, T)
        runs.append((T, float(np.abs(y - ref).max()), e_t, _rms(ref)))
    e_torch = max(r[2] for r in runs)
    for T, err, e_t, rms in runs:
        print("head C %d T %d: hip %.3e torch %.3e (case %.3e) bar %.3e ratio to torch %.2f" % (
            C, T, err, e_t, e_torch, 4.0 * e_torch + 1e-7 * rms, err / e_torch))
    for T, err, e_t, rms in runs:
        assert err <= 4.0 * e_torch + 1e-7 * rms, (T, err, e_torch)


# ---- the cases can fail: wrong variants lie more than 100 bars away ------------------------------------------------------------------

@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("wrong", ["swap_taps", "weight_as_conv", "unpadded_left"])
@pytest.mark.parametrize("case", [(16, 2, 2), (16, 4, 4)], ids=["u2-s2", "u4-s4"])
def test_seam_wrong_variants_are_far(dev, case, wrong):
    Cout, u, s = case
    w = O.seeded_seam_weights(Cout, u, s, seed=7 * u + s)
    rng = np.random.default_rng(u)
    for Tin in (1, NG.seam_tile(Cout, u) + 1):
        x, src = _seam_inputs(rng, 2, Cout, u, s, Tin)
        ref = O.seam(x, *w[:2], u, src, *w[2:], s)
        bar = 4.0 * float(np.abs(_torch_seam(x, w, u, src, s) - ref).max()) + 1e-7 * _rms(ref)
        y = _seam_run(dev, x, w, u, src, s)
        assert np.abs(y - ref).max() <= bar, (Tin, np.abs(y - ref).max(), bar)
        bad = O.seam(x, *w[:2], u, src, *w[2:], s, **{wrong: True})
        assert np.abs(bad - ref).max() > 100 * bar, (Tin, np.abs(bad - ref).max(), bar)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("case", [(16, 2, 1), (16, 8, 2)], ids=["u2", "u8"])
def test_seam_edge_columns_have_a_single_live_tap(dev, case):
    """the first and the last u / 2 output columns of a sequence take their second tap from outside [0, Tin): zero, not a copy
    of the neighbour -- also where the sequence ends inside a tile and at a tile's first column"""
    Cout, u, s = case
    p = u // 2
    w = O.seeded_seam_weights(Cout, u, s, seed=11 * u)
    rng = np.random.default_rng(5 + u)
    tq = NG.seam_tile(Cout, u)
    for Tin in (1, 3, tq, tq + 1):
        x, src = _seam_inputs(rng, 2, Cout, u, s, Tin)
        ref = O.seam(x, *w[:2], u, src, *w[2:], s)
        bar = 4.0 * float(np.abs(_torch_seam(x, w, u, src, s) - ref).max()) + 1e-7 * _rms(ref)
        y = _seam_run(dev, x, w, u, src, s)
        edges = np.r_[0:p, u * Tin - p:u * Tin]
        assert np.abs(y - ref)[:, :, edges].max() <= bar
        assert np.abs(y - ref).max() <= bar
        bad = O.seam(x, *w[:2], u, src, *w[2:], s, replicate_edges=True)
        assert np.abs(bad - ref)[:, :, :p].max() > 100 * bar and np.abs(bad - ref)[:, :, u * Tin - p:].max() > 100 * bar
        assert np.array_equal(bad[:, :, p:u * Tin - p], ref[:, :, p:u * Tin - p])


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_head_slope_is_the_default_not_the_blocks(dev):
    C = 16
    w = O.seeded_head_weights(C, seed=8)
    rng = np.random.default_rng(8)
    for T in (1, NG.head_tile(C) + 1):
        x = rng.standard_normal((2, C, T)).astype(np.float32)
        ref = O.head(x, *w)
        bar = 4.0 * float(np.abs(_torch_head(x, w) - ref).max()) + 1e-7 * _rms(ref)
        y = _head_run(dev, x, w)
        assert np.abs(y - ref).max() <= bar
        bad = O.head(x, *w, slope=O.SLOPE)
        assert np.abs(bad - ref).max() > 100 * bar, (T, np.abs(bad - ref).max(), bar)
        y1 = _head_run(dev, x, w, slope=0.1)                                       # the argument reaches the kernel
        assert np.abs(y1 - bad).max() <= 4.0 * float(np.abs(_torch_head(x, w, 0.1) - bad).max()) + 1e-7 * _rms(bad)


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------

def _wn(m):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.nn.utils.weight_norm(m)


def _seam_modules(Cout=16, u=2, s=2, k=None, pad=None, output_padding=0, noise=None):
    up = torch.nn.ConvTranspose1d(2 * Cout, Cout, 2 * u if k is None else k, u, padding=u // 2 if pad is None else pad,
                                  output_padding=output_padding)
    if noise is None:
        noise = torch.nn.Conv1d(1, Cout, 2 * s, s, padding=s // 2) if s > 1 else torch.nn.Conv1d(1, Cout, 1)
    return up, noise


def _seam_line(up, noise, x, src):
    return up(F.leaky_relu(x, 0.1)) + noise(src)


def _seam_counts():
    return NG.CALLS["seam_hip"], NG.CALLS["seam_reference"]


def _head_counts():
    return NG.CALLS["head_hip"], NG.CALLS["head_reference"]


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_seam_dispatch(dev):
    torch.manual_seed(0)
    x = torch.randn(2, 32, 9)
    blocks0 = NG.CALLS["hip"], NG.CALLS["reference"]
    with torch.no_grad():
        up, noise = _seam_modules()
        src = torch.randn(2, 1, 2 * 2 * 9)
        h0, r0 = _seam_counts()
        y = NG.seam_forward(up, noise, x, src)         # plain modules: the kernel
        assert _seam_counts() == (h0 + 1, r0) and (y - _seam_line(up, noise, x, src)).abs().max() <= 1e-5
        for make in (lambda: (_wn(up), noise), lambda: (torch.nn.utils.remove_weight_norm(up), _wn(noise))):
            a, b = make()                              # a weight-norm hook on either: the torch line, to the bit
            y = NG.seam_forward(a, b, x, src)
            assert _seam_counts() == (h0 + 1, r0 + 1) and torch.equal(y, _seam_line(a, b, x, src))
            r0 += 1
        torch.nn.utils.remove_weight_norm(noise)
        assert NG.seam_forward(up, noise, x, src) is not None and _seam_counts() == (h0 + 2, r0)
        h0 += 2
        others = [_seam_modules(k=6, pad=2),                                       # k = 3 u
                  _seam_modules(u=4, k=4, pad=0),                                  # k = u: another stride / kernel relation
                  _seam_modules(pad=0),                                            # Tout = u Tin + u
                  _seam_modules(u=4, output_padding=1),                            # output_padding 1
                  _seam_modules(noise=torch.nn.Conv1d(1, 16, 6, 3, padding=2)),    # odd noise stride
                  _seam_modules(noise=torch.nn.Conv1d(1, 16, 4, 2, padding=0)),    # unpadded noise conv
                  _seam_modules(Cout=128)]                                         # the 256 -> 128 seam
        for a, b in others:
            xa = torch.randn(2, a.in_channels, 9)
            Tout = a(xa).shape[-1]
            sa = torch.randn(2, 1, (Tout - 1) * b.stride[0] + b.kernel_size[0] - 2 * b.padding[0])
            want = _seam_line(a, b, xa, sa)
            assert want.shape[-1] == Tout
            got = NG.seam_forward(a, b, xa, sa)
            r0 += 1
            assert _seam_counts() == (h0, r0) and torch.equal(got, want)
        up64 = up.double()
        assert NG.seam_forward(up64, noise.double(), x.double(), src.double()).dtype == torch.float64      # float64
        r0 += 1
        assert _seam_counts() == (h0, r0)
        up.float(), noise.float()
        short = src[:, :, :-1]                                                      # a source of another length: torch decides
        with pytest.raises(RuntimeError):
            NG.seam_forward(up, noise, x, short)
        r0 += 1
        assert _seam_counts() == (h0, r0)
    xg = x.clone().requires_grad_(True)                # a gradient is needed: the differentiable torch line
    yg = NG.seam_forward(up, noise, xg, src)
    assert _seam_counts() == (h0, r0 + 1) and yg.requires_grad
    yg.sum().backward()
    assert xg.grad is not None and up.weight.grad is not None
    with torch.no_grad():
        assert NG.seam_forward(up, noise, xg, src) is not None and _seam_counts() == (h0 + 1, r0 + 1)
    assert (NG.CALLS["hip"], NG.CALLS["reference"]) == blocks0                     # the block counters keep their meaning


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_head_dispatch(dev):
    torch.manual_seed(1)
    x = torch.randn(2, 16, 30)
    line = lambda c, v: torch.tanh(c(F.leaky_relu(v)))
    with torch.no_grad():
        post = torch.nn.Conv1d(16, 1, 7, 1, padding=3)
        h0, r0 = _head_counts()
        y = NG.head_forward(post, x)
        assert _head_counts() == (h0 + 1, r0) and (y - line(post, x)).abs().max() <= 1e-6
        for c, v in ((_wn(torch.nn.Conv1d(16, 1, 7, 1, padding=3)), x), (torch.nn.Conv1d(16, 1, 5, 1, padding=2), x),
                     (torch.nn.Conv1d(16, 1, 7, 1, padding=0), x), (torch.nn.Conv1d(16, 2, 7, 1, padding=3), x),
                     (torch.nn.Conv1d(128, 1, 7, 1, padding=3), torch.randn(1, 128, 12)),
                     (torch.nn.Conv1d(16, 1, 7, 1, padding=3, bias=False), x)):
            got = NG.head_forward(c, v)
            r0 += 1
            assert _head_counts() == (h0 + 1, r0) and torch.equal(got, line(c, v))
    xg = x.clone().requires_grad_(True)
    yg = NG.head_forward(post, xg)
    assert _head_counts() == (h0 + 1, r0 + 1) and yg.requires_grad
    with torch.no_grad():
        assert torch.equal(NG.head_forward(post, xg), y) and _head_counts() == (h0 + 2, r0 + 1)


def test_dispatch_keeps_host_tensors_on_torch():
    up, noise = _seam_modules()
    post = torch.nn.Conv1d(16, 1, 7, 1, padding=3)
    x, src = torch.randn(1, 32, 6), torch.randn(1, 1, 24)
    with torch.no_grad():
        s0, h0 = _seam_counts(), _head_counts()
        assert torch.equal(NG.seam_forward(up, noise, x, src), _seam_line(up, noise, x, src))
        xh = torch.randn(1, 16, 12)
        assert torch.equal(NG.head_forward(post, xh), torch.tanh(post(F.leaky_relu(xh))))
        assert _seam_counts() == (s0[0], s0[1] + 1) and _head_counts() == (h0[0], h0[1] + 1)
    with pytest.raises(RuntimeError):
        NG.upsample_stage(x, up.weight, up.bias, 2, src, noise.weight, noise.bias, 2)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_in_place_weight_update_invalidates_the_packed_seam(dev):
    torch.manual_seed(2)
    up, noise = _seam_modules(u=4, s=2)
    x, src = torch.randn(1, 32, 11), torch.randn(1, 1, 88)
    with torch.no_grad():
        y0 = NG.seam_forward(up, noise, x, src)
        assert (y0 - _seam_line(up, noise, x, src)).abs().max() <= 1e-5
        assert torch.equal(NG.seam_forward(up, noise, x, src), y0)                 # the cached table
        up.weight.mul_(-2.0)
        y1 = NG.seam_forward(up, noise, x, src)
        assert (y1 - y0).abs().max() > 1e-2 and (y1 - _seam_line(up, noise, x, src)).abs().max() <= 1e-5
        noise.bias.add_(0.5)
        noise.weight.mul_(3.0)
        y2 = NG.seam_forward(up, noise, x, src)
        assert (y2 - y1).abs().max() > 1e-2 and (y2 - _seam_line(up, noise, x, src)).abs().max() <= 1e-5
        post = torch.nn.Conv1d(16, 1, 7, 1, padding=3)                             # the head reads its weights in place
        xh = torch.randn(1, 16, 20)
        z0 = NG.head_forward(post, xh)
        post.weight.mul_(-1.5)
        z1 = NG.head_forward(post, xh)
        assert (z1 - z0).abs().max() > 1e-2 and (z1 - torch.tanh(post(F.leaky_relu(xh)))).abs().max() <= 1e-6


class _Source(torch.nn.Module):
    """a seeded stand-in for the harmonic source (the reference's draws noise on every call)"""

    def forward(self, f0, upp):
        g = torch.Generator().manual_seed(5)
        return (0.1 * torch.randn(f0.shape[0], f0.shape[1] * upp, 1, generator=g)).to(f0)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_reference_generator_patched_counts_seams_and_head(dev):
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
        for p in list(gen.ups.parameters()) + list(gen.conv_post.parameters()):    # the init's std 0.01 leaves only the biases
            p.mul_(3.0)
        mel, f0 = torch.randn(2, 8, 40), torch.full((2, 40), 220.0)
        gen.remove_weight_norm()
        want = gen(mel, f0)
        exact = gen.double()(mel.double(), f0.double()).numpy()
        gen.float()
        try:
            NG.patch_reference_generator()
            s0, h0 = _seam_counts(), _head_counts()
            got = gen(mel, f0)
            assert _seam_counts() == (s0[0] + 2, s0[1]) and _head_counts() == (h0[0] + 1, h0[1])
            NG.SEAM_TORCH_FASTER[(16, 2)] = None                                   # one seam left to torch, stage by stage
            try:
                again = gen(mel, f0)
            finally:
                del NG.SEAM_TORCH_FASTER[(16, 2)]
            assert _seam_counts() == (s0[0] + 3, s0[1] + 1) and _head_counts() == (h0[0] + 2, h0[1])
        finally:
            NG.unpatch_reference_generator()
        s1, h1 = _seam_counts(), _head_counts()
        assert torch.equal(gen(mel, f0), want)                                     # unpatched: the reference's bits
        assert (_seam_counts(), _head_counts()) == (s1, h1)
    assert got.shape == want.shape == (2, 1, 160)
    bar = 4.0 * float(np.abs(want.numpy() - exact).max()) + 1e-7 * _rms(exact)      # test_resblock.py's bar for the whole generator
    print("generator: hip %.3e, one seam on torch %.3e, bar %.3e, rms %.3f" % (
        np.abs(got.numpy() - exact).max(), np.abs(again.numpy() - exact).max(), bar, _rms(exact)))
    assert np.abs(got.numpy() - exact).max() <= bar and np.abs(again.numpy() - exact).max() <= bar
    assert 0.05 < _rms(exact) < 0.9                    # neither only the biases nor a saturated tanh


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_bad_arguments(dev):
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    assert lib.ddsp_hip_version() == 165
    assert [lib.ddsp_hip_upsample_stage_tile(C, u) for C, u in ((16, 2), (32, 4), (64, 4), (64, 8))] == [128, 128, 128, 64]
    assert lib.ddsp_hip_upsample_stage_tile(128, 2) == 0 and lib.ddsp_hip_upsample_stage_tile(16, 3) == 0
    assert lib.ddsp_hip_output_head_tile(16) == 1024 and lib.ddsp_hip_output_head_tile(128) == 0
    Co, u, s, Tin = 16, 2, 2, 5
    wu, bu, wn, bn = [torch.from_numpy(a) for a in O.seeded_seam_weights(Co, u, s, seed=1)]
    need = lib.ddsp_hip_upsample_stage_pack_bytes(Co, u, s)
    assert need == 4 * (2 * Co * Co * 2 * u + Co + 9 * Co)
    for bad in ((48, u, s), (128, u, s), (Co, 3, s), (Co, 16, s), (Co, u, 3), (Co, u, 0), (Co, u, 8)):
        assert lib.ddsp_hip_upsample_stage_pack_bytes(*bad) == 0, bad
    tab = torch.zeros(need // 4)
    pack = lambda **kw: lib.ddsp_hip_upsample_stage_pack(*[kw.get(n, d) for n, d in (
        ("wu", wu.data_ptr()), ("bu", bu.data_ptr()), ("wn", wn.data_ptr()), ("bn", bn.data_ptr()), ("C", Co), ("u", u), ("s", s),
        ("t", tab.data_ptr()), ("tb", need))])
    for kw, code in (({"tb": need - 4}, -4), ({"C": 24}, -3), ({"u": 6}, -3), ({"s": 3}, -3), ({"wu": None}, -1), ({"bu": None}, -1),
                     ({"wn": None}, -1), ({"bn": None}, -1), ({"t": None}, -1)):
        assert pack(**kw) == code, kw
        assert (tab == 0).all(), kw
    assert pack() == 0
    x, src = torch.randn(2, 2 * Co, Tin), torch.randn(2, 1, s * u * Tin)
    y = torch.full((2, Co, u * Tin), 7.0)
    call = lambda **kw: lib.ddsp_hip_upsample_stage(*[kw.get(n, d) for n, d in (
        ("x", x.data_ptr()), ("src", src.data_ptr()), ("y", y.data_ptr()), ("t", tab.data_ptr()), ("tb", need), ("B", 2), ("C", Co),
        ("T", Tin), ("u", u), ("s", s), ("st", None))])
    for kw, code in (({"C": 128}, -3), ({"C": 24}, -3), ({"u": 3}, -3), ({"u": 16}, -3), ({"u": 0}, -3), ({"s": 3}, -3), ({"s": 0}, -3),
                     ({"s": 8}, -3), ({"T": 0}, -1), ({"T": -4}, -1), ({"T": (1 << 30) + 1}, -3), ({"B": -1}, -1), ({"x": None}, -1),
                     ({"src": None}, -1), ({"y": None}, -1), ({"t": None}, -1), ({"y": x.data_ptr()}, -1),
                     ({"y": src.data_ptr()}, -1), ({"tb": need - 4}, -4), ({"y": y.data_ptr() + 2}, -1)):
        assert call(**kw) == code, kw
        assert (y == 7.0).all(), kw                    # refused before any launch
    assert call(B=0, x=None, src=None, y=None) == 0 and (y == 7.0).all()           # a no-op
    assert call() == 0
    ref = O.seam(x.numpy(), wu.numpy(), bu.numpy(), u, src.numpy(), wn.numpy(), bn.numpy(), s)
    assert np.abs(y.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()

    C, T = 16, 9
    wp, bp = [torch.from_numpy(a) for a in O.seeded_head_weights(C, seed=2)]
    xh = torch.randn(2, C, T)
    yh = torch.full((2, 1, T), 7.0)
    head = lambda **kw: lib.ddsp_hip_output_head(*[kw.get(n, d) for n, d in (
        ("x", xh.data_ptr()), ("w", wp.data_ptr()), ("b", bp.data_ptr()), ("slope", 0.01), ("y", yh.data_ptr()), ("B", 2), ("C", C),
        ("T", T), ("st", None))])
    for kw, code in (({"C": 128}, -3), ({"C": 8}, -3), ({"C": 48}, -3), ({"T": 0}, -1), ({"T": -1}, -1), ({"T": (1 << 40) + 1}, -3),
                     ({"B": -1}, -1), ({"x": None}, -1), ({"w": None}, -1), ({"b": None}, -1), ({"y": None}, -1),
                     ({"y": xh.data_ptr()}, -1), ({"slope": float("nan")}, -1), ({"slope": float("inf")}, -1),
                     ({"y": yh.data_ptr() + 1}, -1)):
        assert head(**kw) == code, kw
        assert (yh == 7.0).all(), kw
    assert head(B=0, x=None, y=None) == 0 and (yh == 7.0).all()
    assert head() == 0
    assert np.abs(yh.numpy() - O.head(xh.numpy(), wp.numpy(), bp.numpy())).max() <= 1e-6


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_unaligned_outputs_take_the_scalar_stores(dev):
    """``out`` one float behind a 16-byte boundary: the seam's U-float stores and the head's 16-byte stores must not be used"""
    Co, u, s, Tin = 16, 4, 1, 7
    w = O.seeded_seam_weights(Co, u, s, seed=4)
    wt = _t(w, dev)
    rng = np.random.default_rng(4)
    x, src = _seam_inputs(rng, 2, Co, u, s, Tin)
    n = 2 * Co * u * Tin
    buf = torch.full((n + 8,), float("nan"))
    out = buf[1:1 + n].view(2, Co, u * Tin)
    y = NG.upsample_stage(torch.from_numpy(x), wt[0], wt[1], u, torch.from_numpy(src), wt[2], wt[3], s, out=out)
    assert y is out and torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + n:]).all()
    assert torch.equal(y, NG.upsample_stage(torch.from_numpy(x), wt[0], wt[1], u, torch.from_numpy(src), wt[2], wt[3], s))
    wh = _t(O.seeded_head_weights(16, seed=5), dev)
    xh = torch.from_numpy(rng.standard_normal((2, 16, 21)).astype(np.float32))
    bufh = torch.full((2 * 21 + 8,), float("nan"))
    outh = bufh[3:3 + 42].view(2, 1, 21)
    yh = NG.output_head(xh, wh[0], wh[1], out=outh)
    assert torch.isnan(bufh[:3]).all() and torch.isnan(bufh[45:]).all() and torch.equal(yh, NG.output_head(xh, wh[0], wh[1]))


# ---- GPU only -------------------------------------------------------------------------------------------------------------------

def _gui_case(dev):
    """the last stage over the GUI's 2.35 s window: 32 channels at 256 columns per frame -> 16 at 512, then the head"""
    frames = 203
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 32, 256 * frames, generator=g).to(dev)
    src = torch.randn(1, 1, 512 * frames, generator=g).to(dev)
    seam = _t(O.seeded_seam_weights(16, 2, 1, seed=6), dev)
    blocks = [([tuple(torch.from_numpy(a).to(dev) for a in pair) for pair in BO.seeded_weights(16, k, 3, seed=9 + k)], (1, 3, 5))
              for k in (3, 7, 11)]
    head = _t(O.seeded_head_weights(16, seed=7), dev)
    return x, src, seam, blocks, head


@pytest.mark.gpu
def test_gpu_call_allocates_only_the_output():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    x, src, seam, _, head = _gui_case(dev)
    h = NG.upsample_stage(x, seam[0], seam[1], 2, src, seam[2], seam[3], 1)        # packs the weights
    NG.output_head(h, head[0], head[1])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    y = NG.upsample_stage(x, seam[0], seam[1], 2, src, seam[2], seam[3], 1)
    mid = torch.cuda.memory_allocated(dev)
    z = NG.output_head(y, head[0], head[1])
    after = torch.cuda.memory_allocated(dev)
    assert mid - before == y.numel() * 4 and after - mid == z.numel() * 4


@pytest.mark.gpu
def test_gpu_graph_replay_is_bit_identical():
    """a seam, the stage's blocks and the head: every launch goes to the caller's stream, one behind the other"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    x, src, seam, blocks, head = _gui_case(dev)

    def run():
        h = NG.upsample_stage(x, seam[0], seam[1], 2, src, seam[2], seam[3], 1)
        return NG.output_head(NG.mrf_stage(h, blocks), head[0], head[1])
    eager = run().clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert out.shape == (1, 1, 512 * 203) and torch.equal(out, eager)
    n = 300                                            # the first columns against the oracle (the cut's reach stays behind them)
    xs, ss = x[:, :, :n].cpu().numpy(), src[:, :, :2 * n].cpu().numpy()
    hh = O.seam(xs, *[t.cpu().numpy() for t in seam[:2]], 2, ss, *[t.cpu().numpy() for t in seam[2:]], 1)
    st = BO.stage(hh, [([tuple(t.cpu().numpy() for t in p) for p in w], d) for w, d in blocks])
    ref = O.head(st, *[t.cpu().numpy() for t in head])
    assert np.abs(eager[:, :, :400].cpu().numpy() - ref[:, :, :400]).max() <= 1e-4
