"""The upsampling seam and the output head (csrc/generator_tail.h) at and past the 65 535-utterance grid limit, by the method of
test_batch_split.py: the ``BATCH_SPLIT`` knob lowers the chunk to 2 and 1 utterances, so that B = 5 gives chunks 2, 2, 1; the
split result must EQUAL the unsplit one bit for bit, the unsplit one meets its parity bar against the float64 oracle, and every
utterance differs from every other (a base of zero cannot pass).  On the GPU the true limit runs: B = 65 537 filled from a pool
of 251 distinct utterances, compared bitwise with the pool's own run."""
import numpy as np
import pytest
import torch

from tests import generator_tail_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_generator_tail import _rms, _t, _torch_head, _torch_seam

from ddsp_svc_amd import nsf_generator as NG  # noqa: E402

SPLITS = (2, 1)
POOL = 251
LIMIT = 65535
NAN = float("nan")


def _rows_differ(a):
    a = np.asarray(a)
    a = a.reshape(a.shape[0], -1)
    for i in range(a.shape[0]):
        for j in range(i + 1, a.shape[0]):
            assert not np.array_equal(a[i], a[j]), (i, j)


def _seam_case(B, Cout, u, s, Tin, seed):
    w = O.seeded_seam_weights(Cout, u, s, seed=seed)
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal((B, 2 * Cout, Tin)).astype(np.float32)
    src = rng.standard_normal((B, 1, s * u * Tin)).astype(np.float32)
    ref = O.seam(x, *w[:2], u, src, *w[2:], s)
    bar = 4.0 * float(np.abs(_torch_seam(x, w, u, src, s) - ref).max()) + 1e-7 * _rms(ref)
    return w, x, src, ref, bar


def _seam_run(wt, x, src, u, s):
    y = torch.full((x.shape[0], x.shape[1] // 2, u * x.shape[2]), NAN, device=x.device)
    assert NG.upsample_stage(x, wt[0], wt[1], u, src, wt[2], wt[3], s, out=y) is y
    return y


def _head_case(B, C, T, seed):
    w = O.seeded_head_weights(C, seed=seed)
    x = np.random.default_rng(seed + 1).standard_normal((B, C, T)).astype(np.float32)
    ref = O.head(x, *w)
    bar = 4.0 * float(np.abs(_torch_head(x, w) - ref).max()) + 1e-7 * _rms(ref)
    return w, x, ref, bar


def _head_run(wt, x):
    y = torch.full((x.shape[0], 1, x.shape[2]), NAN, device=x.device)
    assert NG.output_head(x, wt[0], wt[1], out=y) is y
    return y


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("case", ["tiles", "short"])
def test_seam_split(dev, knobs, case):
    """tiles: Tin = tile + 1, two column tiles meet the batch chunks, s = 2; short: Tin = 3 at u = 4, s = 1"""
    Cout, u, s, Tin = (16, 2, 2, NG.seam_tile(16, 2) + 1) if case == "tiles" else (16, 4, 1, 3)
    w, x, src, ref, bar = _seam_case(5, Cout, u, s, Tin, seed=13)
    wt = _t(w, dev)
    xt, st = torch.from_numpy(x).to(dev), torch.from_numpy(src).to(dev)
    whole = _seam_run(wt, xt, st, u, s)
    assert torch.isfinite(whole).all()
    err = float(np.abs(whole.cpu().numpy().astype(np.float64) - ref).max())
    print("seam case %s: error %.3e, bar %.3e" % (case, err, bar))
    assert err <= bar
    _rows_differ(whole.cpu().numpy())
    _rows_differ(ref)
    for split in SPLITS:
        knobs("BATCH_SPLIT", split)
        part = _seam_run(wt, xt, st, u, s)
        assert torch.isfinite(part).all(), split
        assert torch.equal(part, whole), split


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("T", ["tile+1", 5])
def test_head_split(dev, knobs, T):
    C = 16
    T = NG.head_tile(C) + 1 if T == "tile+1" else T
    w, x, ref, bar = _head_case(5, C, T, seed=17)
    wt = _t(w, dev)
    xt = torch.from_numpy(x).to(dev)
    whole = _head_run(wt, xt)
    assert torch.isfinite(whole).all()
    err = float(np.abs(whole.cpu().numpy().astype(np.float64) - ref).max())
    print("head T %d: error %.3e, bar %.3e" % (T, err, bar))
    assert err <= bar
    _rows_differ(whole.cpu().numpy())
    _rows_differ(ref)
    for split in SPLITS:
        knobs("BATCH_SPLIT", split)
        part = _head_run(wt, xt)
        assert torch.isfinite(part).all(), split
        assert torch.equal(part, whole), split


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.gpu
def test_seam_past_the_grid_limit():
    """B = 65 537 = 65 535 + 2 at Cout = 16, u = 2, s = 1, Tin = 3: 25 MB in, 25 MB out"""
    device = _gpu()
    B, u, s = LIMIT + 2, 2, 1
    w, xp, sp, ref, bar = _seam_case(POOL, 16, u, s, 3, seed=23)
    wt = _t(w, device)
    xpool, spool = torch.from_numpy(xp).to(device), torch.from_numpy(sp).to(device)
    ypool = _seam_run(wt, xpool, spool, u, s)
    assert float(np.abs(ypool.cpu().numpy().astype(np.float64) - ref).max()) <= bar
    _rows_differ(ref)
    idx = torch.arange(B, device=device) % POOL
    y = _seam_run(wt, xpool[idx].contiguous(), spool[idx].contiguous(), u, s)
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx])


@pytest.mark.gpu
def test_head_past_the_grid_limit():
    """B = 65 537 at C = 16, T = 5: 21 MB in, 1.3 MB out"""
    device = _gpu()
    B = LIMIT + 2
    w, xp, ref, bar = _head_case(POOL, 16, 5, seed=29)
    wt = _t(w, device)
    xpool = torch.from_numpy(xp).to(device)
    ypool = _head_run(wt, xpool)
    assert float(np.abs(ypool.cpu().numpy().astype(np.float64) - ref).max()) <= bar
    _rows_differ(ref)
    idx = torch.arange(B, device=device) % POOL
    y = _head_run(wt, xpool[idx].contiguous())
    assert torch.isfinite(y).all()
    assert torch.equal(y, ypool[idx])
