"""The real-time caller's splice (ddsp_svc_amd.splice, csrc/splice.h): SOLA search, crossfade and phase vocoder of gui.py:15-32 and
gui.py:431-456, against the float64 oracle (tests/splice_oracle.py), which is itself pinned to the reference's own callbacks
(tests/golden/splice_*.npz, make_golden_splice.py)."""
import types

import numpy as np
import pytest
import torch

from tests import splice_oracle as O
from tests.backends import BACKENDS, dev  # noqa: F401

EINVAL, ESHAPE, EWS = -1, -3, -4


def _rel_rms(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))


def _signal(n, seed):
    """drifting partials plus noise (the model's output stands in): SOLA has a real optimum to find"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    f0 = 150.0 + 60.0 * np.sin(2 * np.pi * 0.9 * t + rng.uniform(0, 2 * np.pi))
    ph = 2 * np.pi * np.cumsum(f0) / 44100.0
    x = sum(rng.uniform(0.1, 0.5) / h * np.sin(h * ph + rng.uniform(0, 2 * np.pi)) for h in range(1, 8))
    return (x + 0.03 * rng.standard_normal(n)).astype(np.float32)


def _case(B, Bf, C, S, D, seed, extra=37):
    """audio [B, L] and a previous tail [B, C]: the samples at a seeded offset of the search range, scaled and with noise added"""
    L = Bf + C + S + D + extra
    audio, buf = np.empty((B, L), np.float32), np.empty((B, C), np.float32)
    st = L - (Bf + C + S + D)
    for u in range(B):
        rng = np.random.default_rng(seed + 17 * u)
        audio[u] = _signal(L, seed + 17 * u)
        s = int(rng.integers(0, S + 1))
        buf[u] = 0.9 * audio[u, st + s: st + s + C] + 0.05 * rng.standard_normal(C).astype(np.float32)
    return audio, buf


def _windows(C):
    fi, fo = O.gui_windows(C)
    if fi.shape[0] != C:             # torch.arange(0, 1, 1 / C) can hold C + 1 points; the GUI would fail there, the test uses C
        t = np.arange(C, dtype=np.float32) / np.float32(C)
        fi = (np.sin(np.pi * t / 2) ** 2).astype(np.float32)
        fo = (1 - fi).astype(np.float32)
    return fi, fo


# ---- the oracle against the reference's own callbacks (no library) ----------------------------------------------------------
@pytest.mark.parametrize("name", ["splice_plain", "splice_pv", "splice_short"])
def test_oracle_reproduces_reference_callbacks(golden_dir, name):
    z = np.load("%s/%s.npz" % (golden_dir, name))
    Bf, C, S, D, pv = (int(v) for v in z["sizes"])
    buf = np.zeros(C, np.float32)
    for c in range(z["audio"].shape[0]):
        out, nb, sh, r = O.splice(z["audio"][c], buf, z["fade_in"], z["fade_out"], Bf, C, S, D, bool(pv))
        assert sh[0] == z["shift"][c], (c, sh, z["shift"][c])
        if pv:        # the reference's own float32 vocoder: its w * t argument carries ~pi C eps radians
            assert np.max(np.abs(out[0] - z["out"][c])) <= 2e-6 * max(1.0, np.max(np.abs(z["out"][c])))
            assert np.max(np.abs(nb[0] - z["buffer"][c])) <= 2e-6 * max(1.0, np.max(np.abs(z["buffer"][c])))
        else:         # the torch chain's two float32 roundings, reproduced exactly
            assert np.array_equal(out[0].astype(np.float32), z["out"][c]) and np.array_equal(nb[0].astype(np.float32), z["buffer"][c])
        buf = z["buffer"][c]


def test_oracle_reproduces_reference_phase_vocoder(golden_dir):
    z = np.load("%s/splice_pv_direct.npz" % golden_dir)
    for n in (96, 77):
        got = O.phase_vocoder(z["a%d" % n], z["b%d" % n], z["fade_out%d" % n], z["fade_in%d" % n])
        assert _rel_rms(z["out%d" % n], got) <= 1e-5, n


@pytest.mark.parametrize("name", ["splice_plain", "splice_pv", "splice_short"])
def test_restated_torch_chain_reproduces_reference_callbacks(golden_dir, name):
    """AtenSplice / aten_phase_vocoder (the torch side of tools/splice_latency.py) give the reference's bits on the CPU"""
    z = np.load("%s/%s.npz" % (golden_dir, name))
    Bf, C, S, D, pv = (int(v) for v in z["sizes"])
    chain = O.AtenSplice(Bf, C, S, D, torch.from_numpy(z["fade_in"]), torch.from_numpy(z["fade_out"]), bool(pv))
    for c in range(z["audio"].shape[0]):
        outdata = np.zeros((Bf, 2), np.float32)
        assert chain(torch.from_numpy(z["audio"][c].copy()), outdata) == z["shift"][c]
        assert np.array_equal(outdata[:, 0], z["out"][c]) and np.array_equal(outdata[:, 1], z["out"][c])
        assert np.array_equal(chain.tail.numpy(), z["buffer"][c])
    d = np.load("%s/splice_pv_direct.npz" % golden_dir)
    for n in (96, 77):
        t = lambda k: torch.from_numpy(d[k % n])
        assert np.array_equal(O.aten_phase_vocoder(t("a%d"), t("b%d"), t("fade_out%d"), t("fade_in%d")).numpy(), d["out%d" % n])


# ---- the C ABI refuses bad arguments before any launch (no GPU needed) ------------------------------------------------------
def test_splice_abi_argument_errors():
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    p, q, ws = 4096, 8192, 65536                        # never dereferenced: every call below fails its checks first
    need = lib.ddsp_hip_splice_workspace_bytes(2, 1764, 0)
    assert need == 2 * 4104 * 8
    assert lib.ddsp_hip_splice_workspace_bytes(2, 1764, 1) == need + 2 * 883 * 32
    assert lib.ddsp_hip_splice_workspace_bytes(1, 0, 1) == 0 and lib.ddsp_hip_splice_workspace_bytes(0, 64, 0) == 0

    def call(B=1, L=1000, ld=1000, Bf=300, C=128, S=40, D=20, audio=p, bi=p, bo=q, use_pv=0, w=ws, wb=1 << 20):
        return lib.ddsp_hip_sola_splice(audio, ld, B, L, Bf, C, S, D, bi, bo, p, p, use_pv, p, p, w, wb, None)
    assert call(D=0) == EINVAL                          # the reference's [-X:-0] slice is empty
    assert call(Bf=0) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(L=487) == EINVAL                        # L < Bf + C + S + D = 488
    assert call(ld=999) == EINVAL
    assert call(audio=None) == EINVAL
    assert call(bo=p) == EINVAL                         # the tails must be two buffers
    assert call(C=0) == ESHAPE and call(C=16385, L=20000, ld=20000) == ESHAPE
    assert call(S=-1) == ESHAPE and call(S=4097, L=6000, ld=6000) == ESHAPE
    assert call(w=None) == EWS and call(wb=need // 2 - 1) == EWS and call(use_pv=1, wb=4104 * 8) == EWS
    assert call(w=ws + 8) == EINVAL                     # 16-byte alignment
    assert call(B=0) == 0                               # an empty batch is a no-op
    assert lib.ddsp_hip_phase_vocoder(p, p, p, p, 0, p, ws, 1 << 20, None) == EINVAL
    assert lib.ddsp_hip_phase_vocoder(p, p, p, p, 16385, p, ws, 1 << 30, None) == ESHAPE
    assert lib.ddsp_hip_phase_vocoder(p, None, p, p, 64, p, ws, 1 << 20, None) == EINVAL
    assert lib.ddsp_hip_phase_vocoder(p, p, p, p, 64, p, ws, 4104 * 8, None) == EWS


def test_python_refuses_bad_sizes():
    from ddsp_svc_amd import splice
    x, b, w = torch.zeros(1000), torch.zeros(128), torch.ones(128)
    for sizes in [(300, 128, 40, 0), (0, 128, 40, 20), (300, 0, 40, 20), (300, 16385, 40, 20), (300, 128, -1, 20), (300, 128, 4097, 20)]:
        with pytest.raises(ValueError):
            splice.sola_splice(x, b, w, w, *sizes)
        with pytest.raises(ValueError):
            splice.StreamingSplice(1, *sizes, w, w)


# ---- the library on the emulator and the GPU ------------------------------------------------------------------------------
CASES = [  # B, Bf, C, S, D
    (1, 300, 128, 40, 20),
    (3, 64, 161, 33, 7),        # Bf < C, odd C, B = 3
    (2, 200, 97, 0, 5),         # S = 0
    (1, 150, 96, 17, 1),
]


def _check_splice(dev, B, Bf, C, S, D, use_pv, seed):
    from ddsp_svc_amd import splice
    audio, buf = _case(B, Bf, C, S, D, seed)
    fi, fo = _windows(C)
    if use_pv:                  # keep the vocoder's phase differences 1e-4 away from the +-pi wrap (ill-conditioned there)
        _, _, sh0, _ = O.splice(audio, buf, fi, fo, Bf, C, S, D)
        seg = O.segment(audio, Bf, C, S, D)
        for u in range(B):
            assert O.wrap_margin(buf[u], seg[u, sh0[u]: sh0[u] + C], fo, fi) > 1e-4, "pick another seed"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out, nb, sh = splice.sola_splice(t(audio), t(buf), t(fi), t(fo), Bf, C, S, D, use_phase_vocoder=use_pv)
    out, nb, sh = out.cpu().numpy(), nb.cpu().numpy(), sh.cpu().numpy()
    assert out.shape == (B, Bf) and nb.shape == (B, C) and sh.shape == (B,)
    _, _, want_sh, ratio = O.splice(audio, buf, fi, fo, Bf, C, S, D)
    for u in range(B):
        assert sh[u] == want_sh[u] or O.near_tie(ratio[u]), (u, sh[u], want_sh[u])
    want_out, want_nb, _, _ = O.splice(audio, buf, fi, fo, Bf, C, S, D, use_pv, shift=sh)
    got = np.concatenate([out, nb], axis=1)
    want = np.concatenate([want_out, want_nb], axis=1)
    if not use_pv:
        assert np.array_equal(got, want.astype(np.float32))
    else:
        assert np.array_equal(got[:, C:], want[:, C:].astype(np.float32))        # past the crossfade: plain copies
        seg = O.segment(audio, Bf, C, S, D)
        for u in range(B):
            e = _rel_rms(got[u, :C], want[u, :C])
            head = seg[u, sh[u]: sh[u] + C]
            e_torch = _rel_rms(O.aten_phase_vocoder(*(torch.from_numpy(np.ascontiguousarray(v)) for v in (buf[u], head, fo, fi))).numpy(),
                               want[u, :C])
            print("B=%d Bf=%d C=%d S=%d: vocoder rel rms %.2e (the float32 torch chain: %.2e)" % (B, Bf, C, S, e, e_torch))
            assert e <= 1e-6, (u, e)
    return sh


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
@pytest.mark.parametrize("B,Bf,C,S,D", CASES)
def test_sola_splice_against_oracle(dev, B, Bf, C, S, D, use_pv):
    sh = _check_splice(dev, B, Bf, C, S, D, use_pv, seed=100 + C)
    if S > 0:
        assert np.any(sh > 0), "the seeded tails should make the search move"


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
def test_silence_and_zero_tail_give_shift_zero(dev, use_pv):
    from ddsp_svc_amd import splice
    Bf, C, S, D = 100, 64, 30, 10
    fi, fo = (torch.from_numpy(v).to(dev) for v in _windows(C))
    audio, buf = (torch.from_numpy(v).to(dev) for v in _case(2, Bf, C, S, D, seed=5))
    zero_a, zero_b = torch.zeros_like(audio), torch.zeros_like(buf)
    for a, b in [(zero_a, zero_b), (audio, zero_b), (zero_a, buf)]:
        out, nb, sh = splice.sola_splice(a, b, fi, fo, Bf, C, S, D, use_phase_vocoder=use_pv)
        assert sh.cpu().tolist() == [0, 0]
    out, nb, sh = splice.sola_splice(zero_a, zero_b, fi, fo, Bf, C, S, D, use_phase_vocoder=use_pv)
    assert not out.cpu().any() and not nb.cpu().any()


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("n", [1, 2, 77, 96, 1764])
def test_phase_vocoder_alone(dev, n):
    from ddsp_svc_amd import splice
    rng = np.random.default_rng(n)
    fi, fo = _windows(n)
    for _ in range(20):
        a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        if O.wrap_margin(a, b, fo, fi) > 1e-4:
            break
    t = lambda v: torch.from_numpy(v).to(dev)
    got = splice.phase_vocoder(t(a), t(b), t(fo), t(fi)).cpu().numpy()
    want = O.phase_vocoder(a, b, fo, fi)
    e = _rel_rms(got, want)
    print("n=%d: vocoder rel rms %.2e" % (n, e))
    assert e <= 1e-6


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("use_pv", [False, True])
@pytest.mark.parametrize("B", [1, 2])
def test_streaming_session_matches_chained_calls(dev, B, use_pv):
    from ddsp_svc_amd import splice
    Bf, C, S, D = 120, 80, 24, 9
    fi, fo = (torch.from_numpy(v).to(dev) for v in _windows(C))
    blocks = [torch.from_numpy(_case(B, Bf, C, S, D, seed=40 + i)[0]).to(dev) for i in range(5)]
    if B == 1:
        blocks = [x[0] for x in blocks]                 # the GUI's 1-D tensors
    sess = splice.StreamingSplice(B, Bf, C, S, D, fi, fo, use_pv, device=dev)
    buf = torch.zeros(C, device=dev) if B == 1 else torch.zeros(B, C, device=dev)
    first = None
    for i, x in enumerate(blocks):
        want_out, buf, want_sh = splice.sola_splice(x, buf, fi, fo, Bf, C, S, D, use_phase_vocoder=use_pv)
        out, sh = sess(x)
        assert torch.equal(out.cpu(), want_out.cpu()) and torch.equal(sh.cpu(), want_sh.cpu()), i
        assert torch.equal(sess.sola_buffer.cpu().reshape(buf.shape), buf.cpu()), i
        if i == 0:
            first = out.clone().cpu()
    sess.reset()
    out, _ = sess(blocks[0])
    assert torch.equal(out.cpu(), first)
    with pytest.raises(ValueError):
        sess(blocks[0][..., : Bf + C + S + D - 1])


# ---- GPU only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vocoder_at_the_slider_maximum():
    """crossfade 0.15 s at 96 kHz: C = 14 400, search 960, the vocoder on"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for seed in range(900, 920):
        audio, buf = _case(1, 2880, 14400, 960, 1920, seed)
        fi, fo = _windows(14400)
        _, _, sh0, _ = O.splice(audio, buf, fi, fo, 2880, 14400, 960, 1920)
        seg = O.segment(audio, 2880, 14400, 960, 1920)
        if O.wrap_margin(buf[0], seg[0, sh0[0]: sh0[0] + 14400], fo, fi) > 1e-4:
            break
    else:
        pytest.fail("no seed keeps the phase differences away from the wrap")
    _check_splice(torch.device("cuda:0"), 1, 2880, 14400, 960, 1920, True, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("use_pv", [False, True])
def test_streaming_calls_replay_in_two_graphs(use_pv):
    """one graph per parity of the ping-ponged tails, replayed in turn: the chain of eager calls, bit for bit"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddsp_svc_amd import splice
    dev = torch.device("cuda:0")
    Bf, C, S, D = 13230, 1764, 441, 882
    fi, fo = (torch.from_numpy(v).to(dev) for v in _windows(C))
    blocks = [torch.from_numpy(_case(1, Bf, C, S, D, seed=7 + i)[0][0]).to(dev) for i in range(5)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sess = splice.StreamingSplice(1, Bf, C, S, D, fi, fo, use_pv, device=dev)
        want = []
        for x in blocks:                                # eager, from the zero tail
            out, sh = sess(x)
            want.append((out.clone(), sh.clone(), sess.sola_buffer.clone()))
        sess.reset()
        x_static = blocks[0].clone()
        graphs = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
        for g in graphs:
            with torch.cuda.graph(g, stream=s):
                sess(x_static)
        assert sess._cur == 0                           # two captures: back at the first parity
        for i, x in enumerate(blocks):
            x_static.copy_(x)
            graphs[i % 2].replay()
            sess._cur = 1 - sess._cur                   # what the replayed call did to the tails
            out, sh, buf = want[i]
            assert torch.equal(sess.out[0], out) and torch.equal(sess.shift[0], sh) and torch.equal(sess.sola_buffer, buf), i
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_patched_reference_phase_vocoder_runs_on_hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddsp_svc_amd import splice
    calls = []

    def original(a, b, fade_out, fade_in):
        calls.append(a.device.type)
        return O.aten_phase_vocoder(a, b, fade_out, fade_in)
    gui = types.SimpleNamespace(phase_vocoder=original)
    assert splice.patch_reference_splice(gui) is gui and gui.phase_vocoder is not original
    splice.patch_reference_splice(gui)                  # idempotent
    assert gui.phase_vocoder._ddsp_hip_original is original
    fi, fo = _windows(1764)
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(1764).astype(np.float32), rng.standard_normal(1764).astype(np.float32)
    g = lambda v: torch.from_numpy(v).cuda()
    got = gui.phase_vocoder(g(a), g(b), g(fo), g(fi))
    assert calls == [] and got.is_cuda
    assert torch.equal(got, splice.phase_vocoder(g(a), g(b), g(fo), g(fi)))
    cpu = gui.phase_vocoder(*(torch.from_numpy(v) for v in (a, b, fo, fi)))
    assert calls == ["cpu"] and not cpu.is_cuda
