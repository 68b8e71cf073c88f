"""Gradient of the log-mel front-end w.r.t. the waveform (csrc/mel.hip k_mel_bwd + k_mel_bwd_gather, mel.py's autograd node):
what the cascades' DDSP loss, ``F.mse_loss(get_mel(ddsp_wav).transpose(1, 2), gt)``, back-propagates through
(reflow/vocoder.py:149-186, diffusion/vocoder.py:221-301).

Pinning: a float64 adjoint restated here (torch autograd of pad -> stft -> magnitude -> basis -> log-clamp) sits within
``REF_PIN`` of the reference's own float32 gradients (fixture mel_grad.npz, tests/golden/make_golden_mel_grad.py, which
also re-draws every input here).  The HIP path is held against the float64 adjoint: <= 2e-5 relative RMS where every band
of every frame sits >= 1e-3 of the frame's largest (``WELL``); elsewhere within 2x the reference's own float32 deviation
from float64 (the fixture's gradients, or the same float32 torch chain run here) -- the log-mel adjoint divides by the
mel value, so float32 noise in weak bands is amplified alike in every float32 implementation.  Measured on the MI355X: the
HIP path 2.7e-7 .. 4.7e-6 from float64, the reference's float32 autograd 2.9e-7 .. 4.3e-6.  The cascade's control gradients
are held to this synth's backward applied to the float64 adjoint (G64): within 2x the reference's own deviation from G64
plus test_backward_fast.py's 5e-6 (measured: the HIP chain 3e-7 .. 6e-6 per stream, the reference 1.5e-6 .. 3e-5)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.backends import BACKENDS, dev  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_mel_grad as MG  # noqa: E402

SR, HOP = 44100, 512
CFG = dict(sr=44100, n_mels=128, n_fft=2048, win_size=2048, hop_length=512, fmin=40, fmax=16000)
WELL = 2e-5            # HIP vs float64, relative RMS, well-conditioned signals
REF_PIN = 1e-5         # float64 restatement vs the reference's float32 autograd (measured <= 4.3e-6: test_float64_adjoint_*)


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def rel(a, b):
    return rms(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / rms(b)


def _basis():
    return torch.from_numpy(MG.basis())


def log_mel_torch(y, W, clip=1e-5):
    """nvSTFT.py:97-116 (keyshift 0) in torch operators, in y's dtype"""
    T = y.shape[-1]
    pl = (2048 - HOP) // 2
    pr = max((2048 - HOP + 1) // 2, 2048 - T - pl)
    yp = F.pad(y.unsqueeze(1), (pl, pr), mode="reflect" if pr < T else "constant").squeeze(1)
    spec = torch.stft(yp, 2048, hop_length=HOP, win_length=2048, window=torch.hann_window(2048, dtype=y.dtype, device=y.device),
                      center=False, return_complex=True)
    mag = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    return torch.log(torch.clamp(torch.matmul(W.to(y), mag), min=clip))


def vjp_torch(y, R, W, dtype):
    """d sum(log_mel(y) * R) / d y with torch autograd in ``dtype`` (float64: the adjoint the HIP path is held to)"""
    x = y.detach().to(dtype).requires_grad_(True)
    (log_mel_torch(x, W) * R.to(x)).sum().backward()
    return x.grad


def well_conditioned(y, W):
    with torch.no_grad():
        mel = torch.exp(log_mel_torch(y.double(), W))
    top = mel.max(dim=1, keepdim=True).values
    return bool((mel >= 1e-3 * top).all())


def hip_vjp(y, R, dev, W=None, **stft_kw):
    from ddsp_svc_amd import mel as M
    cfg = dict(CFG, **stft_kw)
    stft = M.STFT(**cfg, mel_basis=W) if W is not None else M.STFT(**cfg)
    x = y.to(dev).clone().requires_grad_(True)
    out = stft.get_mel(x)
    assert out.grad_fn is not None
    (g,) = torch.autograd.grad(out, x, R.to(dev))
    return g.cpu()


def bar(y, R, W, ref32=None):
    """WELL where every band sits >= 1e-3 of the frame maximum, else 2x the float32 chain's own deviation from float64"""
    if well_conditioned(y, W):
        return WELL
    g64 = vjp_torch(y, R, W, torch.float64)
    if ref32 is None:
        ref32 = vjp_torch(y, R, W, torch.float32)
    return max(WELL, 2.0 * rel(ref32, g64))


# ---- CPU: the float64 restatement against the reference's float32 autograd ---------------------------------------------------
@pytest.mark.parametrize("tag", sorted(MG.VJP_CASES))
def test_float64_adjoint_against_reference_autograd(golden_dir, tag):
    fx = np.load(os.path.join(golden_dir, "mel_grad.npz"))
    y, R = MG.vjp_case(tag)
    g64 = vjp_torch(y, R, _basis(), torch.float64).numpy()
    ref = fx["vjp_" + tag]
    assert g64.shape == ref.shape
    e = rel(ref, g64)
    print("%s: reference float32 vs float64 adjoint %.3e (well conditioned: %s)" % (tag, e, well_conditioned(y, _basis())))
    assert e <= REF_PIN


# ---- the kernel against the float64 adjoint -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("tag", sorted(MG.VJP_CASES))
def test_mel_vjp_fixture_cases(dev, golden_dir, tag):
    fx = np.load(os.path.join(golden_dir, "mel_grad.npz"))
    y, R = MG.vjp_case(tag)
    W = _basis()
    g = hip_vjp(y, R, dev)
    g64 = vjp_torch(y, R, W, torch.float64)
    assert g.shape == y.shape and g.dtype == torch.float32
    b = bar(y, R, W, torch.from_numpy(fx["vjp_" + tag]))
    e = rel(g.numpy(), g64.numpy())
    print("%s: HIP vs float64 %.3e, bar %.3e" % (tag, e, b))
    assert e <= b


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("B,T,run", [(1, 512 * 7, 1), (3, 512 * 9 + 100, 2), (1, 700, 4), (2, 300, 4), (1, 512 * 33, 3)])
def test_mel_vjp_shapes(dev, B, T, run, knobs):
    """test_mel.py's shape list: odd frame counts, T not a multiple of the hop, constant padding, several runs per utterance"""
    knobs("MEL_RUN", run)
    rng = np.random.default_rng(T)
    t = np.arange(T) / 44100.0
    y = torch.from_numpy((0.4 * np.sin(2 * np.pi * 330.0 * t)[None] + 0.1 * rng.standard_normal((B, T))).astype(np.float32))
    R = torch.from_numpy(rng.standard_normal((B, 128, MG.frames(T))).astype(np.float32))
    W = _basis()
    g = hip_vjp(y, R, dev)
    e, b = rel(g.numpy(), vjp_torch(y, R, W, torch.float64).numpy()), bar(y, R, W)
    print("B %d T %d run %d: HIP vs float64 %.3e, bar %.3e" % (B, T, run, e, b))
    assert e <= b


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_mel_vjp_dense_basis(dev):
    """a basis that is not banded (40 x 1025 weights: too many to stage on chip) reads the dense basis"""
    rng = np.random.default_rng(5)
    W = torch.from_numpy((rng.random((40, 1025)) * 1e-2).astype(np.float32))
    y = torch.from_numpy((0.1 * rng.standard_normal((2, 512 * 6))).astype(np.float32))
    R = torch.from_numpy(rng.standard_normal((2, 40, 6)).astype(np.float32))
    g = hip_vjp(y, R, dev, W=W, n_mels=40)
    e, b = rel(g.numpy(), vjp_torch(y, R, W, torch.float64).numpy()), bar(y, R, W)
    print("dense basis: HIP vs float64 %.3e, bar %.3e" % (e, b))
    assert e <= b


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_silent_stretch_gets_exact_zeros(dev):
    """samples covered only by frames whose every band is clamped (log(clip_val)) receive exactly 0"""
    from ddsp_svc_amd import mel as M
    y, R = MG.vjp_case("speech2s")
    x = y.to(dev).clone().requires_grad_(True)
    out = M.STFT(**CFG).get_mel(x)
    (g,) = torch.autograd.grad(out, x, R.to(dev))
    clamped = (out.detach().cpu() == out.detach().cpu().min()).all(dim=1)[0].numpy()        # [frames]
    assert clamped.sum() >= 10
    T = y.shape[1]
    cover = np.zeros(T + 2 * 768, dtype=bool)                                               # padded positions of live frames
    for j in np.flatnonzero(~clamped):
        cover[j * HOP: j * HOP + 2048] = True
    only_clamped = ~cover[768:768 + T]
    only_clamped[:768 + 1] = False                                                          # (the reflected head folds back)
    only_clamped[T - 770:] = False
    assert only_clamped.sum() > 10000
    gs = g.cpu().numpy()[0]
    assert (gs[only_clamped] == 0).all()
    assert np.abs(gs[~only_clamped]).max() > 0


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_cotangent_and_input_layouts(dev):
    """a transposed cotangent (mse_loss on the transpose(1, 2) view), a stride-0 one (.sum()), a contiguous one; a float64
    input and a sliced one: dtype, shape and values"""
    from ddsp_svc_amd import mel as M
    W = _basis()
    y, _ = MG.vjp_case("t_odd")
    B, T = y.shape
    nf = MG.frames(T)
    stft = M.STFT(**CFG)
    gt = torch.randn(B, nf, 128, generator=torch.Generator().manual_seed(7)) - 5.0
    # mse on the transposed view
    x = y.to(dev).clone().requires_grad_(True)
    F.mse_loss(stft.get_mel(x).transpose(1, 2), gt.to(dev)).backward()
    with torch.no_grad():
        R = (2.0 / gt.numel()) * (log_mel_torch(y.double(), W).transpose(1, 2) - gt.double()).transpose(1, 2)
    g64 = vjp_torch(y, R, W, torch.float64)
    assert rel(x.grad.cpu().numpy(), g64.numpy()) <= 2 * WELL
    # .sum(): an expanded (stride 0) cotangent
    x = y.to(dev).clone().requires_grad_(True)
    stft.get_mel(x).sum().backward()
    g64 = vjp_torch(y, torch.ones(B, 128, nf), W, torch.float64)
    assert rel(x.grad.cpu().numpy(), g64.numpy()) <= 2 * WELL
    # contiguous cotangent, float64 input
    R = torch.randn(B, 128, nf, generator=torch.Generator().manual_seed(8))
    x64 = y.double().to(dev).requires_grad_(True)
    (g,) = torch.autograd.grad(stft.get_mel(x64), x64, R.to(dev))
    assert g.dtype == torch.float64 and g.shape == x64.shape
    g64 = vjp_torch(y, R, W, torch.float64)
    assert rel(g.cpu().numpy(), g64.numpy()) <= 2 * WELL
    # a slice of a longer leaf: autograd scatters the gradient into it
    lead = torch.randn(B, 300, generator=torch.Generator().manual_seed(9))
    big = torch.cat([lead, y], dim=1).to(dev).requires_grad_(True)
    (gb,) = torch.autograd.grad(stft.get_mel(big[:, 300:]), big, R.to(dev))
    assert gb.shape == big.shape
    assert (gb[:, :300] == 0).all()
    assert rel(gb[:, 300:].cpu().numpy(), g64.numpy()) <= 2 * WELL


@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
def test_no_grad_path_is_unchanged(dev):
    """no node and the same bits as the launch of ddsp_hip_mel_spectrogram, under no_grad and for an input without grad"""
    from ddsp_svc_amd import _ffi
    from ddsp_svc_amd import mel as M
    y, _ = MG.vjp_case("t_odd")
    y = y.to(dev)
    stft = M.STFT(**CFG)
    basis, (band, packed), window = stft._tables(y.device)
    B, T = y.shape
    nf = MG.frames(T)
    want = torch.empty(B, nf, 128, device=y.device)
    _ffi.check(_ffi.lib().ddsp_hip_mel_spectrogram(_ffi.ptr(y), B, T, _ffi.ptr(window), 2048, HOP, _ffi.ptr(basis),
                                                   _ffi.ptr(band), _ffi.ptr(packed), packed.numel(), 128, 1e-5,
                                                   _ffi.ptr(want), nf * 128, 1, 128, _ffi.stream_of(y)))
    a = stft.get_mel(y)
    assert a.grad_fn is None and torch.equal(a, want.transpose(1, 2))
    with torch.no_grad():
        b = stft.get_mel(y.clone().requires_grad_(True))
    assert b.grad_fn is None and torch.equal(b, want.transpose(1, 2))
    c = stft.get_mel(y.clone().requires_grad_(True))                                       # the node's forward: same launch
    assert c.grad_fn is not None and torch.equal(c.detach(), want.transpose(1, 2))


# ---- routing --------------------------------------------------------------------------------------------------------------------
def _standin_nvstft(monkeypatch):
    """a stand-in ``nsf_hifigan.nvSTFT``: an STFT class with a torch get_mel (counting its calls) and librosa_mel_fn"""
    pkg = types.ModuleType("nsf_hifigan")
    nv = types.ModuleType("nsf_hifigan.nvSTFT")
    nv.librosa_mel_fn = lambda sr, n_fft, n_mels, fmin, fmax: MG.basis()
    calls = []

    class STFT:
        def __init__(self, sr=22050, n_mels=80, n_fft=1024, win_size=1024, hop_length=256, fmin=20, fmax=11025, clip_val=1e-5):
            self.target_sr, self.n_mels, self.n_fft, self.win_size = sr, n_mels, n_fft, win_size
            self.hop_length, self.fmin, self.fmax, self.clip_val = hop_length, fmin, fmax, clip_val
            self.mel_basis, self.hann_window = {}, {}

        def get_mel(self, y, keyshift=0, speed=1, center=False):
            calls.append((keyshift, y.device.type))
            return log_mel_torch(y, torch.from_numpy(MG.basis()).to(y.device))

    nv.STFT = STFT
    pkg.nvSTFT = nv
    monkeypatch.setitem(sys.modules, "nsf_hifigan", pkg)
    monkeypatch.setitem(sys.modules, "nsf_hifigan.nvSTFT", nv)
    return nv, calls


def test_patched_stft_sends_cpu_gradient_calls_to_the_reference_code(monkeypatch):
    from ddsp_svc_amd import mel as M
    nv, calls = _standin_nvstft(monkeypatch)
    M.patch_reference_stft()
    y = torch.randn(1, 4096, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    out = nv.STFT(44100, 128, 2048, 2048, 512, 40, 16000).get_mel(y)
    assert calls == [(0, "cpu")] and out.grad_fn is not None
    out.sum().backward()
    assert y.grad is not None


def test_standalone_stft_refuses_a_shifted_gradient_call():
    from ddsp_svc_amd import mel as M
    y = torch.randn(1, 4096).requires_grad_(True)
    with pytest.raises(RuntimeError, match="keyshift=0"):
        M.STFT(**CFG).get_mel(y, keyshift=1)
    with pytest.raises(RuntimeError, match="keyshift=0"):
        M.STFT(**CFG).get_mel(y, center=True)


@pytest.mark.gpu
def test_patched_stft_routes_gradient_calls_on_the_gpu(monkeypatch):
    """plain GPU call that needs a gradient -> the HIP node; a shifted one -> the reference's own (differentiable) code;
    a shifted call without a gradient still takes the chirp-z kernel"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddsp_svc_amd import mel as M
    nv, calls = _standin_nvstft(monkeypatch)
    M.patch_reference_stft()
    stft = nv.STFT(44100, 128, 2048, 2048, 512, 40, 16000)
    y = (torch.randn(2, 512 * 12, generator=torch.Generator().manual_seed(2)) * 0.2).cuda().requires_grad_(True)
    out = stft.get_mel(y)
    assert calls == [] and type(out.grad_fn).__name__.startswith("_MelSpectrogram")
    out.sum().backward()
    g64 = vjp_torch(y.detach().cpu(), torch.ones(2, 128, 12), _basis(), torch.float64)
    assert rel(y.grad.cpu().numpy(), g64.numpy()) <= 2 * WELL
    shifted = stft.get_mel(y, keyshift=2)
    assert calls == [(2, "cuda")] and shifted.grad_fn is not None
    with torch.no_grad():
        stft.get_mel(y, keyshift=2)
    assert len(calls) == 1 and len(stft._hip_shifted) == 1


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def test_backward_argument_errors_are_reported_without_a_gpu():
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    B, T = 2, 512 * 9
    need = lib.ddsp_hip_mel_backward_workspace_bytes(B, T, 2048, 512)
    assert need == B * 9 * 2048 * 4
    assert lib.ddsp_hip_mel_backward_workspace_bytes(B, T, 1024, 512) == 0
    assert lib.ddsp_hip_mel_backward_workspace_bytes(B, T, 2048, 256) == 0
    p = ctypes.c_void_p(4096)                                    # never dereferenced: every check precedes the launch

    def call(n_fft=2048, hop=512, ws_bytes=need, audio=p, grad_out=p, grad_audio=p, bins=p, ws=p, n_mels=128):
        return lib.ddsp_hip_mel_spectrogram_backward(audio, B, T, p, n_fft, hop, p, p, p, 1460, bins, n_mels, 1e-5, grad_out,
                                                     9 * 128, 1, 128, grad_audio, ws, ws_bytes, None)
    assert call(n_fft=1024) == -3                                # DDSP_HIP_ESHAPE
    assert call(hop=256) == -3
    assert call(n_mels=2000) == -3
    assert call(n_fft=1) == -1                                   # DDSP_HIP_EINVAL
    assert call(ws_bytes=need - 4) == -4                         # DDSP_HIP_EWS
    assert call(ws=None) == -4
    for kw in ("audio", "grad_out", "grad_audio", "bins"):
        assert call(**{kw: None}) == -1, kw


# ---- the cascade's DDSP loss end to end ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", BACKENDS, indirect=True)
@pytest.mark.parametrize("kind", ["super", "fast"])
def test_cascade_ddsp_loss_gradients(dev, golden_dir, kind):
    """CombSubSuperFast / CombSubFast (infer=False) -> get_mel -> mse against a target mel -> the control gradients, against
    the reference's autograd (fixture)"""
    from ddsp_svc_amd import mel as M
    from ddsp_svc_amd import synth
    fx = np.load(os.path.join(golden_dir, "mel_grad.npz"))
    f0, ctrls, draw, gt = MG.cascade_inputs(kind)
    f0 = f0.to(dev)
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in ctrls.items()}
    keys = MG.SUPER_KEYS if kind == "super" else MG.SUPER_KEYS[:3]
    if kind == "super":
        st = synth.fast_source(f0, SR, HOP)
        sig = synth.combsubsuperfast_synth(f0, st, *[leaves[k] for k in keys], draw.to(dev), torch.hann_window(2048).to(dev),
                                           SR, HOP)
    else:
        st = synth.phase(f0, SR, HOP, infer=False)
        sig = synth.combsubfast_synth(f0, st, *[leaves[k] for k in keys], (draw * 2 - 1).to(dev),
                                      torch.sqrt(torch.hann_window(1024)).to(dev), SR, HOP)
    # the fixture is the reference's float32 chain, and so is this one: each deviates from exact arithmetic in its synth and in
    # its log-mel adjoint.  The yardstick: this synth's backward applied to the float64 torch adjoint of this very signal (G64).
    # Bar per stream: within 2x the reference's own deviation from G64, and never above 5e-6 more than that
    W, s = _basis(), sig.detach().cpu()
    with torch.no_grad():
        R = (2.0 / gt.numel()) * (log_mel_torch(s.double(), W).transpose(1, 2) - gt.double()).transpose(1, 2)
    c64 = vjp_torch(s, R, W, torch.float64).float()
    g64 = torch.autograd.grad(sig, [leaves[k] for k in keys], c64.to(dev), retain_graph=True)
    mel = M.STFT(**CFG).get_mel(sig).transpose(1, 2)
    F.mse_loss(mel, gt.to(dev)).backward()
    for k, y64 in zip(keys, g64):
        ref, y64 = fx[kind + "_grad_" + k], y64.cpu().numpy()
        e, e_ref = rel(leaves[k].grad.cpu().numpy(), y64), rel(ref, y64)
        print("%s %s: HIP vs G64 %.3e, reference vs G64 %.3e, HIP vs reference %.3e" % (
            kind, k, e, e_ref, rel(leaves[k].grad.cpu().numpy(), ref)))
        assert e <= 2.0 * e_ref + 5e-6, k


# ---- GPU: training shapes, reproducibility ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(48, 172 * 512), (32, 441000)])
def test_mel_vjp_training_shapes(B, T):
    """the reflow training batch (configs/reflow.yaml: 48 x 172 frames) and 32 x 10 s against the float64 adjoint (torch,
    float64, on the GPU); two backward calls give the same bits"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddsp_svc_amd import mel as M
    dev = torch.device("cuda:0")
    y = MG.signal(1, T, 31).expand(B, T).contiguous()
    y = (y * torch.linspace(0.5, 1.5, B)[:, None] + 0.01 * torch.randn(B, T, generator=torch.Generator().manual_seed(3))).to(dev)
    R = torch.randn(B, 128, MG.frames(T), generator=torch.Generator().manual_seed(4)).to(dev)
    stft = M.STFT(**CFG)
    x = y.clone().requires_grad_(True)
    out = stft.get_mel(x)
    (g1,) = torch.autograd.grad(out, x, R, retain_graph=True)
    (g2,) = torch.autograd.grad(out, x, R)
    assert torch.equal(g1, g2)
    W = _basis().to(dev)
    g64 = vjp_torch(y, R, W, torch.float64)
    e = rel(g1.cpu().numpy(), g64.cpu().numpy())
    b = WELL if well_conditioned(y, W) else 2.0 * rel(vjp_torch(y, R, W, torch.float32).cpu().numpy(), g64.cpu().numpy())
    print("B %d T %d: HIP vs float64 %.3e, bar %.3e" % (B, T, e, b))
    assert e <= max(b, WELL)
