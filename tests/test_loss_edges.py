"""The spectral loss (ddsp_svc_amd/loss.py, csrc/loss_czt.hip, csrc/loss.hip) at its geometry, fallback, overlap and cache
edges.  tests/test_loss.py and tests/test_fuzz.py hold the loss to its references at shapes where, on a GPU, every
workgroup makes one pass, the fallback kernels never run on values, the gather sees three hops and the table cache nothing.

  1. passes          29 frames whose kinds (plain, silent truth, silent prediction, equal, prediction 80 dB down, the two
                     signals 240 dB apart either way) cycle with period 7, so that every kind meets both halves of a pair
                     and both pass parities of k_sss_czt's double-buffered flags; one workgroup per PAIR against one
                     workgroup per UTTERANCE, bit for bit.
  2. fallback        k_sss_partial / k_sss_final / k_sss_grad on synthetic spectra at their chunk, tile and grid edges, and
                     through SSSLoss (n_fft > 2048, DDSP_HIP_LOSS_TORCH_STFT=1).
  3. overlap gather  k_frames_overlap_add at hops 1, n - 1 and hops that do not divide n, with row strides and accumulate,
                     and past its 4096-block grid.
  4. RSSLoss         one node: either gradient alone and both, a repeated size, row-padded views, a draw above 2048.
  5. table cache     byte budget, LRU order, accounting, a table evicted between forward and backward; graph capture.

Conditioning as in test_both_gradients: a = 0.1 randn, b = 0.7 a + 0.05 randn, eps = 1e-3 wherever a gradient meets float64
(the gradient is discontinuous where S_true == S_pred; eps = 1e-7 puts bins on that edge).  Bars are those of
tests/test_loss.py: spectra 5e-7 of the maximum, a quiet frame 2e-6 of its own maximum, loss 2e-6, gradient 2e-5 relative
rms, the backward transform against the float64 adjoint of the same bin gradients 1e-6, per frame 2e-5 of the larger
gradient of its pair.  Out of scope (neither is an edge of this code): peak ratios beyond 2^60 between the two signals (the
kernel clamps its rescaling there by design) and amplitudes whose squares overflow float32.

Measured on an MI355X (worst err / bar of each group; every case prints its own):
  1. resident workgroups inferred 1021 / 511 / 256 for n = 16 / 601 / 1031; pool B = 3 in 15 chunks per utterance, batches
     of 1536 / 768 / 384 in 1 chunk; all bits equal.  Spectra 2.6e-7 / 5e-7; loss 8.2e-8 / 2e-6; gradients 3.6e-7 / 2e-5 rms,
     1.3e-7 / 1e-6 against the adjoint, 1.7e-7 / 2e-5 for the worst frame of a pair.  Per frame against the eager float64
     composition: 5 or fewer of the 87 frames take 4 e_torch as their bar, the others 2e-5; worst err / bar 0.36 (8.6e-6 /
     2.4e-5); the largest error, 3.0e-5, is the frame with the near-zero bin described in the test (bar 2.6e-4).
  2. synthetic spectra: loss 6.7e-7 / 2e-6 (one bin), gradients 1.3e-7 / 2e-5.  Through SSSLoss: 0.38 of 4 e_torch + 1e-7 at
     the worst; switch on against off 0.62 of it.
  3. gather: 9.1e-6 / 2e-5 against float64, 1.4e-7 / 1e-6 against the adjoint; past the grid cap 1.7e-6 / 2e-5.
  4. RSSLoss: 3.2e-6 / 2e-5."""
import collections
import functools

import numpy as np
import pytest
import torch

from oracle import ddsp_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_loss import _eager, _rel_rms

F32 = np.float32
NAN = float("nan")
EINVAL, ESHAPE, EWS = -1, -3, -4                               # include/ddsp_hip.h
ALPHA, EPS = 0.8, 1e-3
SPEC_BAR, QUIET_BAR, LOSS_BAR, GRAD_BAR, ADJOINT_BAR, FRAME_BAR = 5e-7, 2e-6, 2e-6, 2e-5, 1e-6, 2e-5


def _report(what, err, bar):
    err = float(err)
    print("%-66s err %.3e  bar %.1e  err/bar %.3f" % (what, err, bar, err / bar))
    assert err <= bar, (what, err, bar)                        # (a NaN fails too)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)               # a copy: the cached cases stay as they are


def _pair(rng, B, T):
    a = (rng.standard_normal((B, T)) * 0.1).astype(F32)
    b = (a * 0.7 + rng.standard_normal((B, T)) * 0.05).astype(F32)
    return a, b


def _eager64(a, b, n, hop, alpha=ALPHA, eps=EPS, go=1.0):
    """loss.py:22-31 in float64 torch ops on the host: loss and both gradients of ``go * loss``"""
    rt = torch.from_numpy(np.array(a)).double().requires_grad_(True)
    rp = torch.from_numpy(np.array(b)).double().requires_grad_(True)
    ref = _eager(rt, rp, n, hop, alpha, eps)
    (go * ref).backward()
    return float(ref.detach()), rt.grad.numpy(), rp.grad.numpy()


def _inv_wn(n):
    return 1.0 / float(torch.hann_window(n).double().pow(2).sum().sqrt())        # as loss.Spectrogram


def _tables(n, like):
    """the tables of one size, outside loss.py's cache (section 5 tests that)"""
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    t = torch.empty(lib.ddsp_hip_stft_loss_table_bytes(n) // 4, dtype=torch.float32, device=like.device)
    _ffi.check(lib.ddsp_hip_stft_loss_tables(n, _ffi.ptr(t), _ffi.stream_of(like)))
    return t


def _wave_forward(xt, xp, T, n, hop, tab, eps=EPS, alpha=ALPHA):
    """ddsp_hip_stft_loss on [B, >= T] rows (row stride = ld) -> spectra [2, B, frames, bins], norms, loss; every output and
    the scratch start as NaN"""
    from ddsp_svc_amd import _ffi
    from ddsp_svc_amd._ffi import ptr
    lib = _ffi.lib()
    B, dev = xt.shape[0], xt.device
    assert xt.stride(1) == 1 and xp.stride() == xt.stride()
    frames = lib.ddsp_hip_stft_loss_frames(T, n, hop)
    spec = torch.full((2, B, frames, n // 2 + 1), complex(NAN, NAN), dtype=torch.complex64, device=dev)
    nb = lib.ddsp_hip_stft_loss_scratch_bytes(B, T, n, hop)
    assert nb > 0 and nb % 24 == 0
    scratch = torch.full((nb // 8,), NAN, dtype=torch.float64, device=dev)
    norms, lo = torch.full((B, 2), NAN, device=dev), torch.full((), NAN, device=dev)
    _ffi.check(lib.ddsp_hip_stft_loss(ptr(xt), ptr(xp), B, T, xt.stride(0), n, hop, ptr(tab), _inv_wn(n), eps, alpha,
                                      ptr(scratch), nb, ptr(spec[0]), ptr(spec[1]), ptr(norms), ptr(lo), _ffi.stream_of(xt)))
    return spec, norms, lo


def _wave_backward_code(spec, norms, T, n, hop, tab, go, wrt_true, d, accumulate, ws, ws_ptr=None, ws_bytes=None,
                        eps=EPS, alpha=ALPHA):
    from ddsp_svc_amd import _ffi
    from ddsp_svc_amd._ffi import ptr
    lib = _ffi.lib()
    if ws_bytes is None:
        ws_bytes = 0 if ws is None else ws.numel() * 4
    if ws_ptr is None:
        ws_ptr = ptr(ws)
    return lib.ddsp_hip_stft_loss_backward(ptr(spec[0]), ptr(spec[1]), spec.shape[1], T, n, hop, ptr(tab), ptr(norms),
                                           _inv_wn(n), eps, alpha, ptr(go), wrt_true, ptr(d), d.stride(0), accumulate,
                                           ws_ptr, ws_bytes, _ffi.stream_of(d))


def _wave_backward(*args, **kw):
    from ddsp_svc_amd import _ffi
    _ffi.check(_wave_backward_code(*args, **kw))


def _chunks(B, T, n, hop):
    """chunks per utterance of the forward launch, from the library's own size function"""
    from ddsp_svc_amd import _ffi
    nb = _ffi.lib().ddsp_hip_stft_loss_scratch_bytes(B, T, n, hop)
    assert nb % (24 * B) == 0
    return nb // (24 * B)


# ---- 1. passes and special frames: the same bits in any geometry ---------------------------------------------------------------
KINDS = ("plain", "silent truth", "silent prediction", "equal", "prediction x 1e-4", "prediction x 1e6, truth x 1e-6",
         "prediction x 1e-6, truth x 1e6")
FRAMES = 29
# Utterance u's frame f is of kind (STEP[u] f + PHASE[u]) mod 7.  4 and 7 are coprime and 29 > 28, so within every utterance
# every kind meets every f mod 4 -- both halves of a pair, both parities of the pass that holds the pair when one workgroup
# walks the utterance.  The flags of a pass were last used two passes (four frames) earlier: kind - 4 STEP mod 7 precedes
# kind there, a different predecessor in each of the three utterances.
STEP, PHASE = (1, 2, 3), (0, 3, 5)


def _kind(u, f):
    return (STEP[u] * f + PHASE[u]) % 7


@functools.lru_cache(maxsize=None)
def _pool(n):
    rng = np.random.default_rng(n)
    T = FRAMES * n + 3
    a, b = _pair(rng, 3, T)
    for u in range(3):
        for f in range(FRAMES):
            s, k = slice(f * n, (f + 1) * n), _kind(u, f)
            if k == 1:
                a[u, s] = 0.0
            elif k == 2:
                b[u, s] = 0.0
            elif k == 3:
                b[u, s] = a[u, s]
            elif k == 4:
                b[u, s] *= F32(1e-4)
            elif k == 5:
                b[u, s] *= F32(1e6)
                a[u, s] *= F32(1e-6)
            elif k == 6:
                b[u, s] *= F32(1e-6)
                a[u, s] *= F32(1e6)
    w = torch.hann_window(n, dtype=torch.float64).numpy()
    X64 = lambda x: np.fft.rfft(x[:, :FRAMES * n].reshape(3, FRAMES, n).astype(np.float64) * w, axis=-1)
    loss, gt, gp = _eager64(a, b, n, n)
    case = dict(a=a, b=b, T=T, Xt=X64(a), Xp=X64(b), loss=loss, gt=gt, gp=gp)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _per_frame_err(got, want, n):
    """rms error of every frame over the larger rms of its pair's references (frames 2i, 2i + 1 share one inverse transform:
    tests/test_loss.py, test_full_size_against_eager_composition)"""
    B = got.shape[0]
    g, r = got[:, :FRAMES * n].reshape(B, FRAMES, n), want[:, :FRAMES * n].reshape(B, FRAMES, n)
    rms = np.sqrt((r ** 2).mean(-1))
    yard = np.pad(rms, ((0, 0), (0, FRAMES % 2))).reshape(B, -1, 2).max(-1, keepdims=True).repeat(2, -1).reshape(B, -1)
    return np.sqrt(((g - r) ** 2).mean(-1)) / np.maximum(yard[:, :FRAMES], 1e-300)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("n", [16, 601, 1031])                             # one size per plan: 1024 / 2048 / 4096 points
def test_passes_and_special_frames_same_bits_in_any_geometry(dev, n, knobs):
    """The pool of three utterances alone, one workgroup per pair of frames (15 chunks: every pass is a first pass), and as
    rows b -> pool[b % 3] of a batch so large that one workgroup walks a whole utterance (1 chunk: 15 passes): spectra, norms
    and both gradients agree bit for bit, and the pool's agree with float64.

    The gradient carries 1 / B and 1 / (B frames bins) as float32 factors, so the batch is 3 * 2^k utterances -- the smallest
    such count that is at least max(4, resident) -- and its grad_out 2^k: every product then differs from the pool's by an
    exact power of two that cancels.

    The chunk counts asserted below are the FORWARD launch's (the size function reports those).  k_sss_czt_bwd is cut by its
    own resident count, which no entry point reports: the pool's pairs are one chunk each there too if that count is at
    least 45, and the batch is one chunk per utterance there only if that count does not exceed B.  Should it exceed B (it
    holds half the forward kernel's LDS at the same launch bounds, so up to twice the forward's count is possible), the
    batch's backward takes an utterance in 2 chunks of 8 and 7 passes.  Either way a backward workgroup of the batch makes
    at least 7 passes where one of the pool makes 1, which is what the bit comparison of the gradients rests on."""
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    p = _pool(n)
    T, bins = p["T"], n // 2 + 1
    resident = lib.ddsp_hip_stft_loss_scratch_bytes(1, n * 200000, n, n) // 24    # min(resident, pairs), pairs = 100000
    assert resident >= 1
    B = 3
    while B < max(4, resident) or _chunks(B, T, n, n) != 1:
        B *= 2
        assert B <= 65535
    rounds = -(-15 * 3 // resident)                                         # a chunk per pair: ceil(resident rounds / 3) >= 15
    if rounds > 1:
        knobs("CZT_ROUNDS", rounds)
    pool_chunks = _chunks(3, T, n, n)
    print("n=%d: resident %d, CZT_ROUNDS %d, pool B=3 in %d chunks per utterance, batch B=%d"
          % (n, resident, rounds, pool_chunks, B))
    assert pool_chunks == 15
    a, b = _t(p["a"], dev), _t(p["b"], dev)
    tab = _tables(n, a)

    def run(xt, xp, go):
        spec, norms, lo = _wave_forward(xt, xp, T, n, n, tab)
        g = torch.full((), go, device=dev)
        ds = []
        for wrt_true in (1, 0):
            d = torch.full(xt.shape, NAN, device=dev)
            _wave_backward(spec, norms, T, n, n, tab, g, wrt_true, d, 0, None)
            ds.append(d)
        for name, x in (("spectra", torch.view_as_real(spec)), ("norms", norms), ("loss", lo), ("d true", ds[0]),
                        ("d pred", ds[1])):
            assert bool(torch.isfinite(x).all()), name
        return spec, norms, lo, ds[0], ds[1]

    spec, norms, lo, dt, dp = run(a, b, 1.0)
    if rounds > 1:
        knobs("CZT_ROUNDS", 0)
    big_chunks = _chunks(B, T, n, n)
    print("n=%d: batch B=%d in %d chunk per utterance" % (n, B, big_chunks))
    assert big_chunks == 1
    idx = torch.arange(B, device=dev) % 3
    spec_b, norms_b, lo_b, dt_b, dp_b = run(a[idx].contiguous(), b[idx].contiguous(), B / 3.0)
    assert torch.equal(torch.view_as_real(spec_b), torch.view_as_real(spec[:, idx])), "spectra differ by geometry"
    assert torch.equal(norms_b, norms[idx]), "norms differ by geometry"
    assert torch.equal(dt_b, dt[idx]), "the gradient to x_true differs by geometry"
    assert torch.equal(dp_b, dp[idx]), "the gradient to x_pred differs by geometry"

    # the pool against float64: spectra per frame, to the frame's own size
    got_t, got_p = spec[0].cpu().numpy(), spec[1].cpu().numpy()
    worst = np.zeros(7)
    for u in range(3):
        for f in range(FRAMES):
            k = _kind(u, f)
            et, ep = np.abs(got_t[u, f] - p["Xt"][u, f]).max(), np.abs(got_p[u, f] - p["Xp"][u, f]).max()
            mt, mp = np.abs(p["Xt"][u, f]).max(), np.abs(p["Xp"][u, f]).max()
            if k <= 3:                                                      # both signals at one scale (or one of them silent)
                e = max(et, ep) / (SPEC_BAR * max(mt, mp))
            else:                                                           # each spectrum to ITS OWN size
                e = max(et / mt, ep / mp) / QUIET_BAR
            worst[k] = max(worst[k], e)
            if k == 1:
                assert not got_t[u, f].any(), ("silence is exact", u, f)
            if k == 2:
                assert not got_p[u, f].any(), ("silence is exact", u, f)
            if k == 3:
                assert np.array_equal(got_t[u, f], got_p[u, f]), ("equal frames, equal spectra", u, f)
    for k in range(7):
        bar = SPEC_BAR if k <= 3 else QUIET_BAR
        _report("n=%d spectra, %s frames" % (n, KINDS[k]), worst[k] * bar, bar)
    _report("n=%d loss, pool" % n, abs(float(lo) - p["loss"]) / p["loss"], LOSS_BAR)
    _report("n=%d loss, batch of %d" % (n, B), abs(float(lo_b) - p["loss"]) / p["loss"], LOSS_BAR)
    # ... and per frame with NO frame excused, each frame to the larger gradient of its pair (the yardstick of
    # test_full_size_against_eager_composition), against two references:
    #   the float64 eager composition, which owes the kernels nothing.  d|z| = z / |z| is discontinuous at z = 0 just as the
    #   log term is at S_true = S_pred: a bin far below eps ||w|| has one of the largest gradients of its frame and a direction
    #   that the float32 rounding of ANY transform (1e-7 of the frame's maximum) turns by 1e-7 max / |z|.  In float64, that
    #   much noise on the one spectrum of utterance 1, frame 25 at n = 1031 -- a plain truth (its prediction is 80 dB
    #   down) whose bin 307 is 1.3e-3 of the maximum, S = 0.3 eps -- moves the frame's gradient by 4.7e-5, and by 1.5e-6
    #   when the noise spares that bin; torch's float32
    #   composition errs by 6.4e-5 there on an MI355X, this kernel by 3.0e-5.  So a frame that the float32 torch composition
    #   on the same device holds to a quarter of the bar meets the bar, FRAME_BAR; another one 4 e_torch of that frame, as the
    #   fallback tests do it;
    #   the float64 adjoint of the kernel's own bin gradients, where nothing is ill-conditioned: the transform alone.
    g1 = torch.ones((), device=dev)
    _, gt32, gp32 = _torch32(p["a"], p["b"], n, n, dev)
    for wrt_true, name, x, d, ref, g32 in ((1, "x_true", p["a"], dt, p["gt"], gt32),
                                           (0, "x_pred", p["b"], dp, p["gp"], gp32)):
        d = d.cpu().numpy()
        assert not d[:, FRAMES * n:].any()                                  # the tail is written, with zeros
        _report("n=%d gradient to %s, rel rms" % (n, name), _rel_rms(d, ref), GRAD_BAR)
        fe, e_torch = _per_frame_err(d, ref, n), _per_frame_err(g32, ref, n)
        bars = np.maximum(FRAME_BAR, 4 * e_torch)
        u, f = np.unravel_index((fe / bars).argmax(), fe.shape)
        print("n=%d gradient to %s: %d of %d frames at 4 e_torch, the others at %.0e; largest error %.3e"
              % (n, name, (bars > FRAME_BAR).sum(), bars.size, FRAME_BAR, fe.max()))
        _report("n=%d gradient to %s against float64, worst frame (%s, utterance %d frame %d)"
                % (n, name, KINDS[_kind(u, f)], u, f), fe[u, f], bars[u, f])
        assert (fe <= bars).all()
        adj = _adjoint64(x, _bin_gradients(spec, norms, n, g1, wrt_true), n, n)
        _report("n=%d gradient to %s against the adjoint of its bin gradients" % (n, name), _rel_rms(d, adj), ADJOINT_BAR)
        _report("n=%d gradient to %s against that adjoint, worst frame of its pair" % (n, name),
                _per_frame_err(d, adj, n).max(), FRAME_BAR)


# ---- 2a. the fallback kernels on synthetic spectra -----------------------------------------------------------------------------
def _sss_chunks(B, per):
    return max(1, min(-(-per // 8192), -(-2048 // B)))                      # loss.hip: 8192 bins a chunk, ~2048 workgroups


def _spectral_case(dev, B, per, chunks):
    """k_sss_partial / k_sss_final / k_sss_grad through the C ABI against the float64 formula of loss.hip's header (autograd
    through it, on the same device).  One NaN bin sits behind each spectrum: a kernel that reads one bin too far shows it."""
    from ddsp_svc_amd import _ffi
    from ddsp_svc_amd._ffi import ptr
    lib = _ffi.lib()
    assert chunks == _sss_chunks(B, per)
    nb = lib.ddsp_hip_spectral_loss_scratch_bytes(B, per)
    assert nb == B * chunks * 24, (nb, B, chunks)
    g = torch.Generator().manual_seed(B * 1000003 + per)
    zt = torch.randn(B * per + 1, 2, generator=g)
    zp = 0.7 * zt + 0.05 * torch.randn(B * per + 1, 2, generator=g)
    zt[-1], zp[-1] = NAN, NAN
    zeros_t = zeros_p = ()
    if per >= 3:                                                            # a few bins exactly zero: in one spectrum, in both
        zeros_t = (0, (B // 2) * per + per // 2)
        zeros_p = (B * per - 1, (B // 2) * per + per // 2)
        zt[list(zeros_t)] = 0.0
        zp[list(zeros_p)] = 0.0
    zt, zp = zt.to(dev), zp.to(dev)
    st, sp = torch.view_as_complex(zt)[:-1].view(B, per), torch.view_as_complex(zp)[:-1].view(B, per)
    inv, go = 0.05, 1.5
    scratch = torch.full((nb // 8,), NAN, dtype=torch.float64, device=dev)
    norms, lo = torch.full((B, 2), NAN, device=dev), torch.full((), NAN, device=dev)
    _ffi.check(lib.ddsp_hip_spectral_loss(ptr(st), ptr(sp), B, per, inv, EPS, ALPHA, ptr(scratch), nb, ptr(norms), ptr(lo),
                                          _ffi.stream_of(st)))
    rt = st.to(torch.complex128).requires_grad_(True)
    rp = sp.to(torch.complex128).requires_grad_(True)
    St, Sp = rt.abs() * inv + EPS, rp.abs() * inv + EPS
    nd, ns = torch.linalg.norm(St - Sp, dim=1), torch.linalg.norm(St + Sp, dim=1)
    ref = torch.mean(nd / ns) + ALPHA * torch.mean((St.log() - Sp.log()).abs())
    (go * ref).backward()
    tag = "B=%d per_utt=%d (%d chunks)" % (B, per, chunks)
    _report(tag + " loss", abs(float(lo) - float(ref.detach())) / float(ref.detach()), LOSS_BAR)
    want_norms = torch.stack([nd, ns], 1).detach()
    _report(tag + " norms", float(((norms.double() - want_norms).abs() / want_norms[:, 1:]).max()), LOSS_BAR)
    gov = torch.full((), go, device=dev)
    for wrt_true, r, zeros in ((1, rt, zeros_t), (0, rp, zeros_p)):
        d = torch.full((B * per + 1, 2), NAN, device=dev)
        d[-1] = 7.0
        _ffi.check(lib.ddsp_hip_spectral_loss_backward(ptr(st), ptr(sp), B, per, ptr(norms), inv, EPS, ALPHA, ptr(gov), wrt_true,
                                                       ptr(d), _ffi.stream_of(st)))
        assert bool((d[-1] == 7.0).all()), "a write behind the last bin"
        got, want = d[:-1].double(), torch.view_as_real(r.grad).reshape(-1, 2)
        assert bool(torch.isfinite(got).all())
        e = float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
        _report(tag + " gradient to the %s spectrum" % ("true" if wrt_true else "predicted"), e, GRAD_BAR)
        for z in zeros:
            assert not d[z].any(), "a zero bin gets a zero gradient"


SPECTRAL = [(B, per, _sss_chunks(1, per)) for per in (1, 1023, 1024, 1025, 8191, 8192, 8193, 3 * 8192 + 5) for B in (1, 3)]
SPECTRAL += [(B, 5, 1) for B in (255, 256, 257, 513)]                       # k_sss_final's b += 256 loop
SPECTRAL += [(1, 1024 * 1024 + 3, 129)]                                     # k_sss_grad's grid of 1024 blocks, four more trips


def test_spectral_cases_expect_these_chunk_counts():
    assert [c for _, _, c in SPECTRAL] == [1] * 12 + [2, 2, 4, 4] + [1] * 4 + [129]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B,per,chunks", SPECTRAL)
def test_fallback_kernels_on_synthetic_spectra(dev, B, per, chunks):
    _spectral_case(dev, B, per, chunks)


@pytest.mark.gpu
def test_fallback_kernels_where_the_workgroup_clamp_binds():
    """B per_utt > 2048 * 8192: sss_chunks gives 2048 / B chunks, not per_utt / 8192 -- here 2 chunks of 8193 bins where the
    bin rule alone would give 3"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, per = 1100, 2 * 8192 + 1
    assert B * per > 2048 * 8192 and -(-per // 8192) == 3
    _spectral_case(torch.device("cuda:0"), B, per, 2)


# ---- 2b. the fallback through SSSLoss ------------------------------------------------------------------------------------------
def _sss_both(f, a, b, dev):
    xt, xp = _t(a, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
    loss = f(xt, xp)
    loss.backward()
    return type(loss.grad_fn).__name__, float(loss.detach()), xt.grad.cpu().numpy(), xp.grad.cpu().numpy()


def _torch32(a, b, n, hop, dev):
    """the same composition in float32 torch ops on ``dev``: its error against float64 is the yardstick of the fallback, whose
    STFT is torch's float32 one"""
    xt, xp = _t(a, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
    w = torch.hann_window(n, dtype=torch.float32, device=dev)
    sp = lambda x: torch.stft(x, n, hop_length=hop, win_length=n, window=w, center=False,
                              return_complex=True).abs() / w.pow(2).sum().sqrt() + EPS
    St, Sp = sp(xt), sp(xp)
    loss = torch.mean(torch.linalg.norm(St - Sp, dim=(1, 2)) / torch.linalg.norm(St + Sp, dim=(1, 2))) \
        + ALPHA * torch.nn.functional.l1_loss(St.log(), Sp.log())
    loss.backward()
    return float(loss.detach()), xt.grad.cpu().numpy(), xp.grad.cpu().numpy()


def _fallback_bars(a, b, n, hop, dev):
    want, gt, gp = _eager64(a, b, n, hop)
    l32, gt32, gp32 = _torch32(a, b, n, hop, dev)
    bars = (4 * abs(l32 - want) / want + 1e-7, 4 * _rel_rms(gt32, gt) + 1e-7, 4 * _rel_rms(gp32, gp) + 1e-7)
    return (want, gt, gp), bars


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("n_fft,overlap", [(2049, 0.0), (2049, 0.75), (3000, 0.0), (3000, 0.75)])
def test_fallback_above_2048_against_float64(dev, n_fft, overlap):
    """overlap 0: the [B, frames, bins] layout of the batched rfft; 0.75: torch.stft's [B, bins, frames]"""
    from ddsp_svc_amd import loss as L
    f = L.SSSLoss(n_fft, ALPHA, overlap, eps=EPS).to(dev)
    T = n_fft + 3 * f.hop_length + 11
    a, b = _pair(np.random.default_rng(n_fft), 2, T)
    (want, gt, gp), bars = _fallback_bars(a, b, n_fft, f.hop_length, dev)
    node, loss, dt, dp = _sss_both(f, a, b, dev)
    assert "_SpectralLossFunction" in node
    tag = "n_fft=%d overlap=%.2f" % (n_fft, overlap)
    _report(tag + " loss", abs(loss - want) / want, bars[0])
    _report(tag + " gradient to x_true", _rel_rms(dt, gt), bars[1])
    _report(tag + " gradient to x_pred", _rel_rms(dp, gp), bars[2])


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B", [1, 3])
def test_fallback_behind_the_environment_switch(dev, B, monkeypatch):
    from ddsp_svc_amd import loss as L
    n_fft = 300
    f = L.SSSLoss(n_fft, ALPHA, 0.5, eps=EPS).to(dev)
    T = n_fft + 4 * f.hop_length + 7
    a, b = _pair(np.random.default_rng(B), B, T)
    (want, gt, gp), bars = _fallback_bars(a, b, n_fft, f.hop_length, dev)
    monkeypatch.delenv("DDSP_HIP_LOSS_TORCH_STFT", raising=False)
    off = _sss_both(f, a, b, dev)
    monkeypatch.setenv("DDSP_HIP_LOSS_TORCH_STFT", "1")
    on = _sss_both(f, a, b, dev)
    assert "_WaveLossFunction" in off[0] and "_SpectralLossFunction" in on[0]
    tag = "n_fft=300 B=%d switch on" % B
    _report(tag + " loss", abs(on[1] - want) / want, bars[0])
    _report(tag + " gradient to x_true", _rel_rms(on[2], gt), bars[1])
    _report(tag + " gradient to x_pred", _rel_rms(on[3], gp), bars[2])
    _report(tag + " against off, loss", abs(on[1] - off[1]) / want, bars[0])
    _report(tag + " against off, gradient to x_true", _rel_rms(on[2], off[2].astype(np.float64)), bars[1])
    _report(tag + " against off, gradient to x_pred", _rel_rms(on[3], off[3].astype(np.float64)), bars[2])


# ---- 3. the overlap gather -----------------------------------------------------------------------------------------------------
def _adjoint64(x, G, n, hop):
    """float64 adjoint of the STFT: the gradient of the signal for the bin gradients G [B, frames, bins]"""
    xx = torch.from_numpy(np.array(x)).double().requires_grad_(True)
    w = torch.hann_window(n, dtype=torch.float64)
    X = torch.stft(xx, n, hop_length=hop, win_length=n, window=w, center=False, return_complex=True)
    X.backward(G.cpu().to(torch.complex128).transpose(1, 2))
    return xx.grad.numpy()


def _bin_gradients(spec, norms, n, go, wrt_true):
    from ddsp_svc_amd import _ffi
    from ddsp_svc_amd._ffi import ptr
    G = torch.empty_like(spec[1])
    B, frames, bins = G.shape
    _ffi.check(_ffi.lib().ddsp_hip_spectral_loss_backward(ptr(spec[0]), ptr(spec[1]), B, frames * bins, ptr(norms), _inv_wn(n),
                                                          EPS, ALPHA, ptr(go), wrt_true, ptr(G), _ffi.stream_of(G)))
    return G


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("n,hop", [(7, 1), (7, 3), (7, 6), (64, 1), (64, 63), (601, 150), (1031, 1030)])
def test_overlap_gather_hops_strides_and_accumulate(dev, n, hop):
    """T = 7 hop + n + 5, row strides T + 3.  The five extra samples hold 5 // hop more frames and leave 5 % hop uncovered:
    at hop 1 -- (7, 1), (64, 1) -- there is NO tail (13 frames cover every sample), so the two tail assertions below are
    empty there and only the pad is checked; (7, 3) has 9 frames and 2 uncovered samples, the other cases 8 frames and 5."""
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    B = 2
    T = 7 * hop + n + 5                                                     # eight frames and five samples more:
    frames = 8 + 5 // hop                                                   # whole hops of those are frames too (hop 1, 3),
    tail = 5 % hop                                                          # the rest is a tail that no frame covers
    ld = T + 3
    a, b = _pair(np.random.default_rng(1000 * n + hop), B, T)
    assert lib.ddsp_hip_stft_loss_frames(T, n, hop) == frames and (frames - 1) * hop + n + tail == T
    bufs = [torch.full((B, ld), NAN, device=dev) for _ in range(2)]         # the pad columns are NaN
    bufs[0][:, :T], bufs[1][:, :T] = _t(a, dev), _t(b, dev)
    xt, xp = bufs[0][:, :T], bufs[1][:, :T]
    tab = _tables(n, xt)
    spec, norms, lo = _wave_forward(xt, xp, T, n, hop, tab)
    go = torch.full((), 2.5, device=dev)
    want, gt, gp = _eager64(a, b, n, hop, go=2.5)
    tag = "n=%d hop=%d" % (n, hop)
    _report(tag + " loss", abs(float(lo) - want) / want, LOSS_BAR)
    need = lib.ddsp_hip_stft_loss_backward_ws_bytes(B, T, n, hop)
    assert need == B * frames * n * 4
    base = _t(np.random.default_rng(5).standard_normal((B, ld)).astype(F32), dev)
    for wrt_true, x, ref in ((1, a, gt), (0, b, gp)):
        who = "x_true" if wrt_true else "x_pred"
        ws = torch.full((need // 4,), NAN, device=dev)
        d = torch.full((B, ld), 7.0, device=dev)
        _wave_backward(spec, norms, T, n, hop, tab, go, wrt_true, d, 0, ws)
        got = d.cpu().numpy()
        assert (got[:, T:] == 7.0).all(), "the pad columns of d_x are not the kernel's"
        assert not got[:, T - tail:T].any(), "the uncovered tail is written, with zeros"
        _report(tag + " gradient to %s against float64" % who, _rel_rms(got[:, :T], ref), GRAD_BAR)
        adj = _adjoint64(x, _bin_gradients(spec, norms, n, go, wrt_true), n, hop)
        _report(tag + " gradient to %s against the adjoint of its bin gradients" % who, _rel_rms(got[:, :T], adj), ADJOINT_BAR)
        d1 = base.clone()
        ws.fill_(NAN)
        _wave_backward(spec, norms, T, n, hop, tab, go, wrt_true, d1, 1, ws)
        assert torch.equal(d1[:, :T], base[:, :T] + d[:, :T]), "accumulate = 1 is buffer + gradient, bit for bit"
        assert torch.equal(d1[:, T - tail:], base[:, T - tail:]), "accumulate = 1 leaves the tail and the pad alone"


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_overlap_gather_refusals(dev):
    from ddsp_svc_amd import _ffi
    n, hop, B, frames = 7, 3, 2, 8
    T = (frames - 1) * hop + n + 2
    a, b = _pair(np.random.default_rng(73), B, T)
    xt, xp = _t(a, dev), _t(b, dev)
    tab = _tables(n, xt)
    spec, norms, _ = _wave_forward(xt, xp, T, n, hop, tab)
    go = torch.ones((), device=dev)
    need = B * frames * n * 4
    assert _ffi.lib().ddsp_hip_stft_loss_backward_ws_bytes(B, T, n, hop) == need
    ws = torch.zeros(need // 4 + 4, device=dev)
    d = torch.full((B, T), 7.0, device=dev)
    assert _wave_backward_code(spec, norms, T, n, hop, tab, go, 0, d, 0, ws, ws_bytes=need - 4) == EWS
    assert _wave_backward_code(spec, norms, T, n, hop, tab, go, 0, d, 0, None, ws_bytes=need) == EWS
    assert ws.data_ptr() % 16 == 0
    assert _wave_backward_code(spec, norms, T, n, hop, tab, go, 0, d, 0, ws, ws_ptr=ws.data_ptr() + 4, ws_bytes=need) == EINVAL
    assert _wave_backward_code(spec, norms, T, n, n + 1, tab, go, 0, d, 0, ws) == ESHAPE             # hop > n
    assert bool((d == 7.0).all()), "a refused call writes nothing"
    assert _wave_backward_code(spec, norms, T, n, hop, tab, go, 0, d, 0, ws, ws_bytes=need) == 0


def _gather_past_the_grid_cap(dev):
    """n = 512, hop = 256, T = 4096 * 256 + 517: the gather's grid stops at 4096 blocks of 256 samples, so the samples from
    1 048 576 on are a block's second trip"""
    n, hop, T = 512, 256, 4096 * 256 + 517
    a, b = _pair(np.random.default_rng(4096), 1, T)
    xt, xp = _t(a, dev), _t(b, dev)
    tab = _tables(n, xt)
    spec, norms, lo = _wave_forward(xt, xp, T, n, hop, tab)
    assert spec.shape[2] == 4097
    want, _, gp = _eager64(a, b, n, hop)
    _report("n=512 hop=256 T=%d loss" % T, abs(float(lo) - want) / want, LOSS_BAR)
    ws = torch.full((4097 * n,), NAN, device=dev)
    d = torch.full((1, T), NAN, device=dev)
    _wave_backward(spec, norms, T, n, hop, tab, torch.ones((), device=dev), 0, d, 0, ws)
    got = d.cpu().numpy()
    assert np.isfinite(got).all() and not got[:, 4096 * hop + n:].any()
    for name, s in (("the last 2000 samples", slice(T - 2000, T)),
                    ("2000 samples around 1 048 576", slice((1 << 20) - 1000, (1 << 20) + 1000))):
        _report("n=512 hop=256 gradient to x_pred, " + name, _rel_rms(got[:, s], gp[:, s]), GRAD_BAR)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_overlap_gather_past_its_grid_cap(dev):
    _gather_past_the_grid_cap(dev)


# ---- 4. RSSLoss as one node ----------------------------------------------------------------------------------------------------
RSS_B = 2


def _nan_fresh_memory(monkeypatch):
    """every buffer the loss allocates with torch.empty starts as NaN: one that is read (accumulated into) before it is
    written shows it"""
    real = torch.empty

    def empty(*args, **kw):
        t = real(*args, **kw)
        return t.fill_(NAN) if t.is_floating_point() or t.is_complex() else t
    monkeypatch.setattr(torch, "empty", empty)


@functools.lru_cache(maxsize=None)
def _rss_case(sizes, overlap):
    T = 2 * max(sizes) + 40
    a, b = _pair(np.random.default_rng(sum(sizes)), RSS_B, T)
    want = float(np.mean([O.sss_loss(a, b, n, ALPHA, overlap, eps=EPS) for n in sizes]))
    gp = np.mean([O.sss_loss_backward(a, b, n, ALPHA, overlap, eps=EPS) for n in sizes], axis=0)
    each = [_eager64(a, b, n, int(n * (1 - overlap))) for n in sizes]       # the oracle has no gradient to x_true
    gt = np.mean([e[1] for e in each], axis=0)
    assert abs(np.mean([e[0] for e in each]) - want) <= 1e-12 * want        # the two float64 references agree
    assert _rel_rms(np.mean([e[2] for e in each], axis=0), gp) <= 1e-9
    for v in (a, b, gt, gp):
        v.setflags(write=False)
    return a, b, want, gt, gp


def _rss(dev, monkeypatch, sizes, overlap, xt, xp):
    from ddsp_svc_amd import loss as L
    rss = L.RSSLoss(2, 4096, len(sizes), ALPHA, overlap, EPS, device=dev)
    monkeypatch.setattr(torch, "randint", lambda *a, **k: torch.tensor(sizes))
    loss = rss(xp, xt)                                                      # loss.py:46: (x_pred, x_true)
    wanted = [x for x in (xt, xp) if x.requires_grad]
    return rss, loss, torch.autograd.grad(loss, wanted) if wanted else ()


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("overlap", [0.0, 0.5])
@pytest.mark.parametrize("sizes", [(300, 300, 512), (16, 601, 1031)])
def test_rss_loss_either_gradient_and_both(dev, sizes, overlap, monkeypatch):
    """a repeated size; one size per plan (the scales add into one gradient buffer, with the gather when frames overlap)"""
    a, b, want, gt, gp = _rss_case(sizes, overlap)
    _nan_fresh_memory(monkeypatch)
    got = {}
    for need_t, need_p in ((True, False), (False, True), (True, True)):
        xt, xp = _t(a, dev).requires_grad_(need_t), _t(b, dev).requires_grad_(need_p)
        rss, loss, grads = _rss(dev, monkeypatch, list(sizes), overlap, xt, xp)
        assert "RandomScaleWaveLoss" in type(loss.grad_fn).__name__
        assert sorted(rss.lossdict) == sorted(set(sizes))
        got[need_t, need_p] = (float(loss.detach()),) + tuple(grads)
    tag = "sizes %s overlap %.1f" % (list(sizes), overlap)
    for key, v in got.items():
        _report(tag + " loss (gradients %s)" % (key,), abs(v[0] - want) / want, LOSS_BAR)
    _report(tag + " gradient to x_true alone", _rel_rms(got[True, False][1].cpu().numpy(), gt), GRAD_BAR)
    _report(tag + " gradient to x_pred alone", _rel_rms(got[False, True][1].cpu().numpy(), gp), GRAD_BAR)
    assert torch.equal(got[True, True][1], got[True, False][1]), "x_true's gradient differs when x_pred's is wanted too"
    assert torch.equal(got[True, True][2], got[False, True][1]), "x_pred's gradient differs when x_true's is wanted too"
    assert got[True, True][0] == got[True, False][0] == got[False, True][0]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("overlap", [0.0, 0.5])
def test_rss_loss_reads_row_padded_views_in_place(dev, overlap, monkeypatch):
    sizes = (16, 601, 1031)
    a, b, want, gt, gp = _rss_case(sizes, overlap)
    T = a.shape[1]
    _nan_fresh_memory(monkeypatch)
    bufs = [torch.full((RSS_B, T + 5), NAN, device=dev) for _ in range(2)]
    bufs[0][:, :T], bufs[1][:, :T] = _t(a, dev), _t(b, dev)
    xt, xp = bufs[0][:, :T].requires_grad_(True), bufs[1][:, :T].requires_grad_(True)
    assert xt.stride() == xp.stride() == (T + 5, 1)
    _, loss, grads = _rss(dev, monkeypatch, list(sizes), overlap, xt, xp)
    assert "RandomScaleWaveLoss" in type(loss.grad_fn).__name__
    ct, cp = _t(a, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
    _, closs, cgrads = _rss(dev, monkeypatch, list(sizes), overlap, ct, cp)
    assert torch.equal(loss.detach(), closs.detach()) and torch.equal(grads[0], cgrads[0]) and torch.equal(grads[1], cgrads[1])
    assert bool(torch.isnan(bufs[0][:, T:]).all()) and bool(torch.isnan(bufs[1][:, T:]).all())
    tag = "row-padded views, overlap %.1f" % overlap
    _report(tag + " loss", abs(float(loss.detach()) - want) / want, LOSS_BAR)
    _report(tag + " gradient to x_true", _rel_rms(grads[0].cpu().numpy(), gt), GRAD_BAR)
    _report(tag + " gradient to x_pred", _rel_rms(grads[1].cpu().numpy(), gp), GRAD_BAR)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_rss_loss_with_a_size_above_the_plans(dev, monkeypatch):
    """a draw that mixes an in-kernel size with one above 2048: the per-scale loop, both paths in one value"""
    from ddsp_svc_amd import loss as L
    sizes, T = [300, 2049], 2 * 2049 + 40
    a, b = _pair(np.random.default_rng(2349), RSS_B, T)
    xt, xp = _t(a, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
    rss, loss, grads = _rss(dev, monkeypatch, sizes, 0.0, xt, xp)
    assert "RandomScaleWaveLoss" not in type(loss.grad_fn).__name__
    ct, cp = _t(a, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
    singles = [L.SSSLoss(n, ALPHA, 0.0, EPS).to(dev)(ct, cp) for n in sizes]
    assert "_WaveLossFunction" in type(singles[0].grad_fn).__name__ and "_SpectralLossFunction" in type(singles[1].grad_fn).__name__
    mean = (0. + singles[0] + singles[1]) / 2
    assert torch.equal(loss.detach(), mean.detach())
    cgrads = torch.autograd.grad(mean, (ct, cp))
    assert torch.equal(grads[0], cgrads[0]) and torch.equal(grads[1], cgrads[1])
    each = [O.sss_loss(a, b, n, ALPHA, 0.0, eps=EPS) for n in sizes]
    want = float(np.mean(each))
    # each path to its own bar, weighted by its share of the value; 1.2e-7 for the float32 sum and division behind them
    bar = (LOSS_BAR * each[0] + _fallback_bars(a, b, 2049, 2049, dev)[1][0] * each[1]) / (each[0] + each[1]) + 1.2e-7
    _report("sizes [300, 2049] loss", abs(float(loss.detach()) - want) / want, bar)
    short = _t(a[:, :2048], dev)
    with pytest.raises(RuntimeError):                                       # shorter than one frame of 2049 (torch.stft)
        L.SSSLoss(2049, ALPHA, 0.0, EPS).to(dev)(short, short)
    with pytest.raises(RuntimeError):
        _rss(dev, monkeypatch, sizes, 0.0, short, short)


# ---- 5. the table cache --------------------------------------------------------------------------------------------------------
def _fresh_cache(monkeypatch, budget):
    from ddsp_svc_amd import loss as L
    monkeypatch.setattr(L, "_CZT_TABLES", collections.OrderedDict())
    monkeypatch.setattr(L, "_czt_tables_held", 0)
    monkeypatch.setattr(L, "_CZT_TABLES_BYTES", budget)
    return L


def _cache_is_consistent(L, n_keys=None):
    assert L._czt_tables_held == sum(t.numel() * 4 for t in L._CZT_TABLES.values())
    if len(L._CZT_TABLES) >= 2:
        assert L._czt_tables_held <= L._CZT_TABLES_BYTES
    if n_keys is not None:
        assert [k[2] for k in L._CZT_TABLES] == n_keys, list(L._CZT_TABLES)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_table_cache_budget_order_and_accounting(dev, monkeypatch):
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    size = lib.ddsp_hip_stft_loss_table_bytes
    # what the budgets below rely on, whatever the tables' layout: two small tables fit the budget of the large one, and of
    # the three small ones any two fit the budget of the larger two but not all three
    assert 8 < size(16) < size(20) < size(24) < size(601) and size(16) + size(20) <= size(601) + 8
    a, b = _pair(np.random.default_rng(601), 2, 1300)
    xt = _t(a, dev)

    def evaluate(L, n, need_grad=False):
        xp = _t(b, dev).requires_grad_(need_grad)
        return L.SSSLoss(n, ALPHA, 0.0, EPS).to(dev)(xt, xp), xp

    def held_backward(budget):
        """forward at 16, then 20 and 601, then the backward pass of 16"""
        L = _fresh_cache(monkeypatch, budget)
        loss, xp = evaluate(L, 16, True)
        _cache_is_consistent(L, [16])
        evaluate(L, 20)
        _cache_is_consistent(L, [16, 20])                                   # two entries, inside the budget
        assert L._czt_tables(16, xt) is L._CZT_TABLES[(str(xt.device), _ffi.stream_of(xt), 16)]
        _cache_is_consistent(L, [20, 16])                                   # a re-used key moves to the end
        evaluate(L, 601)
        return L, loss, xp

    # the budget just above one table of the largest size drawn: that table displaces both others, the older one first
    L, loss, xp = held_backward(size(601) + 8)
    _cache_is_consistent(L, [601])
    grad, = torch.autograd.grad(loss, xp)                                   # the node holds its table: eviction does not free it
    _cache_is_consistent(L, [601])
    for n in (1, 2049):                                                     # outside the plans: None, and nothing added
        assert L._czt_tables(n, xt) is None
    _cache_is_consistent(L, [601])
    L, loss2, xp2 = held_backward(64 << 20)
    _cache_is_consistent(L, [20, 16, 601])
    grad2, = torch.autograd.grad(loss2, xp2)
    assert torch.equal(loss.detach(), loss2.detach()) and torch.equal(grad, grad2)
    # room for two of the three: the least recently USED key is dropped, not the oldest
    L = _fresh_cache(monkeypatch, size(20) + size(24) + 8)
    for n in (16, 20):
        evaluate(L, n)
    assert L._czt_tables(16, xt) is not None
    _cache_is_consistent(L, [20, 16])
    evaluate(L, 24)
    _cache_is_consistent(L, [16, 24])
    evaluate(L, 20)                                                         # 16 + 24 + 20 is over: 16 goes, 24 + 20 fits
    _cache_is_consistent(L, [24, 20])


@pytest.mark.gpu
def test_table_cache_under_graph_capture_and_streams(monkeypatch):
    """A table first needed while a graph is captured exists only after a replay: it is not cached.  The captured chain has
    no parallel branches."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    L = _fresh_cache(monkeypatch, 64 << 20)
    a, b = _pair(np.random.default_rng(28), 2, 500)
    xt, xp = _t(a, dev), _t(b, dev)
    warm = L.SSSLoss(24, ALPHA, 0.0, EPS).to(dev)(xt, xp)                   # the same plan: the launcher's geometry is known
    f = L.SSSLoss(28, ALPHA, 0.0, EPS).to(dev)
    torch.cuda.synchronize()
    _cache_is_consistent(L, [24])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = f(xt, xp)
    _cache_is_consistent(L, [24])                                           # no entry for 28, under any stream
    eager = f(xt, xp)
    _cache_is_consistent(L, [24, 28])
    torch.cuda.synchronize()
    for _ in range(2):
        captured.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager), (float(captured), float(eager))
    assert float(eager) > 0 and float(warm) > 0
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = f(xt, xp)
    side.synchronize()
    _cache_is_consistent(L, [24, 28, 28])
    k_main, k_side = list(L._CZT_TABLES)[1:]
    assert k_main[:2] == (str(dev), torch.cuda.current_stream(dev).cuda_stream) and k_side[:2] == (str(dev), side.cuda_stream)
    assert k_main[1] != k_side[1] and L._CZT_TABLES[k_main] is not L._CZT_TABLES[k_side]
    assert torch.equal(L._CZT_TABLES[k_main], L._CZT_TABLES[k_side]) and torch.equal(other, eager)
