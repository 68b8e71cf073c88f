"""The splice kernels (csrc/splice.h) at their tiling edges, on exact ties and on strided batches, against the float64 oracle
(tests/splice_oracle.py).  tests/test_splice.py holds the kernels to the oracle at sizes that never cross a tile; here:

  search grid        S / 64 + 1 workgroups of 4 waves x 16 candidates: an optimum planted at a chosen offset on both sides of
                     every 64-candidate workgroup edge, of the argmax's 256- and 1024-thread strides, at s = 0, at s = S (the
                     segment read then ends exactly at L - D), at the maximum S = 4096, with off = 0 and with D = 1.  The shift
                     is asserted exactly: the oracle shows first that no other candidate is within 1e-6 of the best.
  exact ties         a periodic segment makes candidates s0, s0 + P, s0 + 2P ... bit-identical; the first must win, in the
                     strided loop of one thread (P = 128, 512), between threads and between workgroups (P = 100, 300, 7).
  workspace          the C ABI on a workspace of +inf and outputs of sentinels: a candidate never written, or an argmax that
                     reads one entry too many, moves the shift.
  vocoder chunks     the 1024-sample DFT chunks, the 1024-bin synthesis stages and the 64-item grids, at and next to their
                     edges, with a per-sample bar beside the rms one.
  strides            row-sliced [B, L] views (stride(0) > L) through sola_splice and StreamingSplice.

NaN or inf in the audio is out of scope: torch.argmax takes a NaN as the maximum, the kernel's ``>`` never does, and the
reference's own output is garbage there."""
import functools

import numpy as np
import pytest
import torch

from tests import splice_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401
from tests.test_splice import _rel_rms, _signal, _windows

F32 = np.float32


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)       # a copy: the cached cases stay as they are


def _oracle(audio, buf, Bf, C, S, D, shift=None):
    """the oracle's plain and vocoder splices of one case (the search is shared) and the vocoder's wrap margins"""
    fi, fo = _windows(C)
    out, nb, sh, ratio = O.splice(audio, buf, fi, fo, Bf, C, S, D, shift=shift)
    out_pv, nb_pv, _, _ = O.splice(audio, buf, fi, fo, Bf, C, S, D, True, shift=sh)
    seg = O.segment(audio, Bf, C, S, D)
    margin = [O.wrap_margin(buf[u], seg[u, sh[u]: sh[u] + C], fo, fi) for u in range(audio.shape[0])]
    return dict(audio=audio, buf=buf, fi=fi, fo=fo, sizes=(Bf, C, S, D), shift=sh, ratio=ratio, margin=margin,
                want={False: np.concatenate([out, nb], axis=1), True: np.concatenate([out_pv, nb_pv], axis=1)})


def _assert_splice(case, use_pv, out, nb, sh):
    """shift exactly the case's; out / new buffer at the bars of tests/test_splice.py"""
    Bf, C, S, D = case["sizes"]
    B = case["audio"].shape[0]
    out, nb, sh = out.cpu().numpy(), nb.cpu().numpy(), sh.cpu().numpy()
    assert out.shape == (B, Bf) and nb.shape == (B, C) and sh.shape == (B,)
    assert sh.tolist() == case["shift"].tolist(), (sh, case["shift"])
    got, want = np.concatenate([out, nb], axis=1), case["want"][use_pv]
    if not use_pv:
        assert np.array_equal(got, want.astype(F32))
        return
    assert np.array_equal(got[:, C:], want[:, C:].astype(F32))                   # past the crossfade: plain copies
    for u in range(B):
        assert case["margin"][u] > 1e-4, "pick another seed: a phase difference sits on the +-pi wrap"
        e = _rel_rms(got[u, :C], want[u, :C])
        print("Bf=%d C=%d S=%d row %d: vocoder rel rms %.2e" % (Bf, C, S, u, e))
        assert e <= 1e-6, (u, e)


def _splice(dev, case, use_pv, audio=None):
    from ddsp_svc_amd import splice
    a = _t(case["audio"], dev) if audio is None else audio
    return splice.sola_splice(a, _t(case["buf"], dev), _t(case["fi"], dev), _t(case["fo"], dev), *case["sizes"],
                              use_phase_vocoder=use_pv)


# ---- 1. an optimum planted at a chosen offset, across the search tiling ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted(Bf, C, S, D, stars, seed, extra=37):
    """tests/test_splice.py's _case with the offsets passed in: row u's tail is 0.9 seg[s* : s* + C] plus noise"""
    B, L = len(stars), Bf + C + S + D + extra
    audio, buf = np.empty((B, L), F32), np.empty((B, C), F32)
    for u, s in enumerate(stars):
        rng = np.random.default_rng(seed + 17 * u)
        audio[u] = _signal(L, seed + 17 * u)
        buf[u] = 0.9 * audio[u, extra + s: extra + s + C] + 0.05 * rng.standard_normal(C).astype(F32)
    case = _oracle(audio, buf, Bf, C, S, D)
    for u, s in enumerate(stars):                       # the premises of an exact shift assertion; never a skip
        assert int(np.argmax(case["ratio"][u])) == s == case["shift"][u], "pick another seed: the oracle's optimum moved"
        assert not O.near_tie(case["ratio"][u]), "pick another seed: the oracle's two best ratios are within 1e-6"
    return case


PLANTED = [  # Bf, C, S, D, s* per row, seed, extra
    (40, 33, 63, 7, (0,), 1, 37),
    (100, 64, 63, 7, (63,), 1, 37),
    (150, 100, 64, 7, (63,), 1, 37),
    (40, 33, 64, 7, (64,), 1, 37),                      # the last workgroup holds this one candidate
    (100, 64, 65, 7, (64,), 1, 37),
    (150, 100, 65, 7, (65,), 1, 37),
    (40, 33, 255, 7, (255,), 1, 37),                    # S + 1 = 256: the plain argmax's one full pass
    (100, 64, 256, 7, (255,), 1, 37),
    (150, 100, 256, 7, (256,), 1, 37),                  # thread 0's second pass
    (40, 33, 1023, 7, (1023,), 1, 37),
    (100, 64, 1024, 7, (1024,), 1, 37),                 # the vocoder argmax's second pass
    (150, 100, 1025, 7, (1024,), 1, 37),
    (40, 33, 1025, 7, (1025,), 1, 37),
    (100, 64, 4096, 7, (0,), 1, 37),                    # the documented maximum
    (150, 100, 4096, 7, (2048,), 1, 37),
    (40, 33, 4096, 7, (4096,), 1, 37),
    (90, 100, 200, 7, (5, 70, 199), 1, 37),             # B = 3, each row's optimum in another workgroup
    (100, 64, 64, 7, (64,), 1, 0),                      # L = Bf + C + S + D: off = 0
    (100, 64, 65, 1, (65,), 1, 37),                     # D = 1
    (60, 33, 70, 1, (70,), 1, 0),                       # both, the optimum last: the read ends at the row's last sample but one
]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
@pytest.mark.parametrize("Bf,C,S,D,stars,seed,extra", PLANTED)
def test_planted_optimum_across_the_search_tiling(dev, Bf, C, S, D, stars, seed, extra, use_pv):
    case = _planted(Bf, C, S, D, stars, seed, extra)
    assert case["audio"].shape[1] - (Bf + C + S + D) == extra
    _assert_splice(case, use_pv, *_splice(dev, case, use_pv))


# ---- 2. exact ties go to the first index ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tied(Bf, C, S, D, P, s0s, seed, extra=37):
    """the C + S searched samples of each row repeat with period P exactly (seg[i] = base[i mod P]) and the tail is
    0.9 seg[s0 : s0 + C] with no noise: candidates s0, s0 + P, s0 + 2P ... see the same numbers in the same lanes in the same
    order, so their ratios are bit-identical, and by Cauchy-Schwarz nothing beats them.  What follows the searched samples is
    not periodic, so a later member of the class would also give another output."""
    B, L = len(s0s), Bf + C + S + D + extra
    audio, buf = np.empty((B, L), F32), np.empty((B, C), F32)
    for u, s0 in enumerate(s0s):
        assert 0 < s0 < P
        rng = np.random.default_rng(seed + 17 * u)
        audio[u] = 0.3 * rng.standard_normal(L).astype(F32)
        audio[u, extra: extra + C + S] = (0.3 * rng.standard_normal(P).astype(F32))[np.arange(C + S) % P]
        buf[u] = F32(0.9) * audio[u, extra + s0: extra + s0 + C]
    case = _oracle(audio, buf, Bf, C, S, D, shift=np.array(s0s))
    for u, s0 in enumerate(s0s):
        r = case["ratio"][u]
        tied = np.zeros(S + 1, bool)
        tied[s0::P] = True
        assert tied.sum() >= 2
        best = r[s0]
        assert best > 0 and np.all(np.abs(r[tied] - best) <= 1e-13 * best), "the tied class is not tied in the oracle"
        assert np.max(r[~tied]) < best * (1 - 1e-6), "pick another seed: a candidate outside the class is a near tie"
    return case


TIED = [  # Bf, C, S, D, P, s0 per row, seed
    (90, 77, 700, 7, 100, (37, 81), 1),                 # across workgroups, the threads of the strided loop and the tree
    (90, 120, 1500, 7, 300, (123, 250), 1),             # the same for the 1024-thread argmax
    (50, 33, 40, 7, 7, (3, 5), 1),                      # one wave, six ties
    (90, 77, 700, 7, 128, (37, 100), 1),                # s0, s0 + 256, s0 + 512 meet in ONE thread of the 256-thread loop
    (90, 120, 1500, 7, 512, (123, 400), 1),             # s0, s0 + 1024 in one thread of the 1024-thread loop
]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
@pytest.mark.parametrize("Bf,C,S,D,P,s0s,seed", TIED)
def test_exact_ties_resolve_to_the_first_index(dev, Bf, C, S, D, P, s0s, seed, use_pv):
    case = _tied(Bf, C, S, D, P, s0s, seed)
    _assert_splice(case, use_pv, *_splice(dev, case, use_pv))


# ---- 3. a poisoned workspace through the C ABI ---------------------------------------------------------------------------------
RATIO_STRIDE = 4104                                     # doubles per utterance (include/ddsp_hip.h)
SENTINEL = -12345.0


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
@pytest.mark.parametrize("S,stars,seed", [(0, (0, 0), 1), (40, (11, 29), 1), (63, (50, 7), 1), (64, (20, 63), 1), (4096, (3000, 77), 1)])
def test_poisoned_workspace_through_the_c_abi(dev, S, stars, seed, use_pv):
    """every ratio entry starts at +inf (not NaN: the argmax's ``>`` would step over it), every output at a sentinel.  Only
    entries 0 .. S may change, to the oracle's ratios (float64 sums of exact products in another order: 1e-12 relative);
    the shift and the outputs are the oracle's, so no candidate went unwritten and the argmax read nothing past S."""
    from ddsp_svc_amd import _ffi
    Bf, C, D, B = 70, 50, 3, 2
    case = _planted(Bf, C, S, D, stars, seed)
    lib = _ffi.lib()
    audio, buf, fi, fo = (_t(case[k], dev) for k in ("audio", "buf", "fi", "fo"))
    L = audio.shape[1]
    need = int(lib.ddsp_hip_splice_workspace_bytes(B, C, int(use_pv)))
    assert need % 8 == 0 and need >= B * RATIO_STRIDE * 8
    ws = torch.full((need // 8,), float("inf"), dtype=torch.float64, device=dev)
    out = torch.full((B, Bf), SENTINEL, dtype=torch.float32, device=dev)
    nb = torch.full((B, C), SENTINEL, dtype=torch.float32, device=dev)
    sh = torch.full((B,), -7, dtype=torch.int64, device=dev)
    _ffi.check(lib.ddsp_hip_sola_splice(audio.data_ptr(), L, B, L, Bf, C, S, D, buf.data_ptr(), nb.data_ptr(), fi.data_ptr(),
                                        fo.data_ptr(), int(use_pv), out.data_ptr(), sh.data_ptr(), ws.data_ptr(), need,
                                        _ffi.stream_of(audio)))
    _assert_splice(case, use_pv, out, nb, sh)
    assert not (out.cpu() == SENTINEL).any() and not (nb.cpu() == SENTINEL).any()
    ratio = ws.cpu().numpy()[: B * RATIO_STRIDE].reshape(B, RATIO_STRIDE)
    assert np.all(np.isposinf(ratio[:, S + 1:])), "the search wrote past candidate S"
    got, want = ratio[:, : S + 1], case["ratio"]
    assert np.all(np.isfinite(got)), "a candidate was never written"
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    print("S=%d: ratios within %.2e relative of the oracle's" % (S, err))
    assert err <= 1e-12


# ---- 4. the vocoder's chunk and grid edges -------------------------------------------------------------------------------------
PV_PER_SAMPLE_BAR = 2e-7                                # worst sample's error over the oracle's peak; see the test below


@functools.lru_cache(maxsize=None)
def _pv_case(n):
    rng = np.random.default_rng(n)
    fi, fo = _windows(n)
    for _ in range(20):
        a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
        if O.wrap_margin(a, b, fo, fi) > 1e-4:
            break
    else:
        pytest.fail("no draw keeps the phase differences away from the wrap")
    return a, b, fo, fi, O.phase_vocoder(a, b, fo, fi)


def _per_sample(x, ref):
    """worst sample's error over the reference's peak"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


def _check_phase_vocoder(dev, n):
    from ddsp_svc_amd import splice
    a, b, fo, fi, want = _pv_case(n)
    got = splice.phase_vocoder(*(_t(v, dev) for v in (a, b, fo, fi))).cpu().numpy()
    e, worst = _rel_rms(got, want), _per_sample(got, want)
    print("n=%d: vocoder rel rms %.2e, worst sample %.2e of the peak" % (n, e, worst))
    assert e <= 1e-6
    assert worst <= PV_PER_SAMPLE_BAR


PV_EDGES = [63, 64, 65, 126, 127, 128, 1023, 1024, 1025, 2047, 2048, 2049]


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("n", PV_EDGES)
def test_phase_vocoder_at_chunk_and_grid_edges(dev, n):
    """The 64-bin / 64-sample grids (n = 126 .. 128: K = 64, 64, 65 bins), the 1024-sample DFT chunks (n = 1023 .. 1025) and the
    1024-bin synthesis stages (n = 2047 .. 2049: K = 1024, 1025, 1025), where both kernels restart their integer twiddle index.

    The rms bar is the contract's 1e-6.  A global rms can hide a few bad samples (one chunk's first bins, say), so each sample
    is also held to PV_PER_SAMPLE_BAR of the oracle's peak.  Measured over these twelve sizes, worst sample over the oracle's peak:
      the kernels on the emulator          2.8e-8 .. 5.13e-8 (the largest at n = 1025), about the rounding of the float32 output
      the kernels on the MI355X            2.8e-8 .. 6.31e-8 (the largest at n = 1024); 3.28e-8 at n = 16 384
      the float32 torch chain (O.aten_phase_vocoder)   1.02e-6 (n = 64) .. 4.90e-5 (n = 2049)
    The bar is 4 x the kernels' own worst, 2e-7: a fifth of the torch chain's best size and 1/250 of its worst, so a chain of
    float32 accuracy fails it at every size here."""
    _check_phase_vocoder(dev, n)


def test_per_sample_bar_is_below_the_float32_torch_chain():
    """the per-sample bar says something only while the float32 torch chain (O.aten_phase_vocoder) misses it, at every size"""
    for n in PV_EDGES:
        a, b, fo, fi, want = _pv_case(n)
        e = _per_sample(O.aten_phase_vocoder(*(torch.from_numpy(v.copy()) for v in (a, b, fo, fi))).numpy(), want)
        print("n=%d: the float32 torch chain's worst sample %.2e of the peak" % (n, e))
        assert PV_PER_SAMPLE_BAR < e, n


@pytest.mark.gpu
def test_phase_vocoder_at_the_documented_maximum():
    """n = 16 384: 16 DFT chunks and 9 synthesis stages of 8193 bins"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check_phase_vocoder(torch.device("cuda:0"), 16384)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_sola_splice_with_two_synthesis_stages(dev):
    """C = 2050: K = 1026 bins, the second 1024-bin stage holds two; three DFT chunks"""
    case = _planted(100, 2050, 70, 7, (64, 13), 1)
    _assert_splice(case, True, *_splice(dev, case, True))


# ---- 5. strided batches ----------------------------------------------------------------------------------------------------------
def _row_sliced(audio, dev):
    """audio [B, L] as a view big[:, 5 : 5 + L] of a wider tensor: contiguous rows, stride(0) = L + 11"""
    B, L = audio.shape
    big = torch.full((B, L + 11), 1e3, dtype=torch.float32, device=dev)            # what a wrong row stride would read
    big[:, 5: 5 + L] = _t(audio, dev)
    view = big[:, 5: 5 + L]
    assert view.stride() == (L + 11, 1) and not (B > 1 and view.is_contiguous())
    return view


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
@pytest.mark.parametrize("stars", [(5, 70, 199), (133,)])
def test_row_sliced_batch_matches_contiguous(dev, stars, use_pv):
    case = _planted(90, 100, 200, 7, stars, 1)
    view = _row_sliced(case["audio"], dev)
    got = _splice(dev, case, use_pv, audio=view)
    want = _splice(dev, case, use_pv, audio=view.contiguous())
    assert all(torch.equal(g.cpu(), w.cpu()) for g, w in zip(got, want))
    _assert_splice(case, use_pv, *got)


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
def test_row_sliced_batch_through_a_streaming_session(dev, use_pv):
    from ddsp_svc_amd import splice
    Bf, C, S, D = 90, 100, 200, 7
    blocks = [_planted(Bf, C, S, D, (5, 70, 199), seed)["audio"] for seed in (1, 2, 3)]
    fi, fo = (_t(v, dev) for v in _windows(C))
    strided = splice.StreamingSplice(3, Bf, C, S, D, fi, fo, use_pv, device=dev)
    packed = splice.StreamingSplice(3, Bf, C, S, D, fi, fo, use_pv, device=dev)
    for i, x in enumerate(blocks):
        view = _row_sliced(x, dev)
        out, sh = strided(view)
        want_out, want_sh = packed(view.contiguous())
        assert torch.equal(out.cpu(), want_out.cpu()) and torch.equal(sh.cpu(), want_sh.cpu()), i
        assert torch.equal(strided.sola_buffer.cpu(), packed.sola_buffer.cpu()), i
        if i > 0:
            assert strided.sola_buffer.cpu().any()
