"""Generate tests/golden/mel_grad.npz by RUNNING THE REFERENCE on CPU (float32 autograd): the gradient of
``nsf_hifigan.nvSTFT.STFT.get_mel`` w.r.t. the waveform (nvSTFT.py:73-117, keyshift 0, 44.1 kHz NSF-HiFiGAN configuration),
and the cascades' DDSP loss (reflow/vocoder.py:149-186, diffusion/vocoder.py:221-301) through it:
``F.mse_loss(get_mel(ddsp_wav).transpose(1, 2), gt)`` back into the controls of CombSubSuperFast / CombSubFast (``infer=False``).

Only runs where the reference checkout is present; librosa is absent, so the oracle's Slaney filterbank is injected for
``librosa_mel_fn`` as make_golden.py does.  Every input is re-drawn from the seeds below (``vjp_case``, ``cascade_inputs``;
tests/test_mel_backward.py imports them), so the fixture holds the reference's gradients only:
  vjp_<tag>          d sum(get_mel(y) * R) / d y for a seeded cotangent R, per case of VJP_CASES
  <kind>_grad_<key>  d mse / d control stream, kind in (super, fast)
Usage:  ``python tests/golden/make_golden_mel_grad.py``
"""
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

SR, HOP, N_FFT, N_MELS, FMIN, FMAX = 44100, 512, 2048, 128, 40, 16000
# tag -> (B, T, seed, silent stretch [start, stop) or None)
VJP_CASES = {
    "speech2s": (1, 2 * SR, 11, (30000, 52000)),     # harmonics + noise, a silent stretch (clamped frames)
    "t_odd": (2, HOP * 9 + 100, 12, None),           # T not a multiple of the hop
    "t1000": (2, 1000, 13, None),                    # reflect: the two mirrored regions overlap
    "t700": (2, 700, 14, None),                      # constant padding (pad_right >= T)
    "t300": (2, 300, 15, None),                      # constant padding, one frame
}
CASCADE = {"super": (2, 5, 21), "fast": (2, 5, 22)}  # kind -> (B, frames, seed)
SUPER_KEYS = ("harmonic_magnitude", "harmonic_phase", "noise_magnitude", "noise_phase")


def basis():
    from oracle import ddsp_oracle as O
    return O.mel_filterbank_slaney(SR, N_FFT, N_MELS, FMIN, FMAX)


def signal(B, T, seed, silent=None):
    """harmonics of a gliding 110..220 Hz tone with noise, float32 [B, T]"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64) / SR
    rows = []
    for b in range(B):
        f0 = 110.0 * (1 + b) * (1 + 0.3 * t)
        ph = 2 * np.pi * torch.cumsum(f0 / SR, 0)
        y = sum(0.3 / k * torch.sin(k * ph + k) for k in range(1, 30))
        rows.append(y + 0.05 * torch.randn(T, generator=g, dtype=torch.float64))
    y = torch.stack(rows).float()
    if silent is not None:
        y[:, silent[0]:silent[1]] = 0.0
    return y


def frames(T):
    pad_left = (N_FFT - HOP) // 2
    pad_right = max((N_FFT - HOP + 1) // 2, N_FFT - T - pad_left)
    return (T + pad_left + pad_right - N_FFT) // HOP + 1


def vjp_case(tag):
    """(audio [B, T], cotangent [B, n_mels, frames]) float32"""
    B, T, seed, silent = VJP_CASES[tag]
    y = signal(B, T, seed, silent)
    R = torch.randn(B, N_MELS, frames(T), generator=torch.Generator().manual_seed(seed + 100))
    return y, R


def cascade_inputs(kind):
    """f0_frames [B, F, 1], controls (dict of [B, F, n]), the exciter noise draw (torch.randn_like for CombSubSuperFast,
    torch.rand_like for CombSubFast) and the target mel gt [B, F, n_mels], float32"""
    from oracle import ddsp_oracle as O
    B, Fr, seed = CASCADE[kind]
    f0 = torch.from_numpy(O.synth_f0(B, Fr, SR, HOP, seed=seed)).float()
    g = torch.Generator().manual_seed(seed + 1)
    n = N_FFT // 2 + 1 if kind == "super" else HOP + 1
    keys = SUPER_KEYS if kind == "super" else SUPER_KEYS[:3]
    ctrls = {}
    for k in keys:
        if k.endswith("magnitude"):
            ctrls[k] = -1.0 + 0.5 * torch.randn(B, Fr, n, generator=g)
        else:
            ctrls[k] = torch.randn(B, Fr, n, generator=g)
    draw = torch.randn(B, Fr * HOP, generator=g) if kind == "super" else torch.rand(B, Fr * HOP, generator=g)
    gt = -6.0 + 2.0 * torch.randn(B, Fr, N_MELS, generator=g)
    return f0, ctrls, draw, gt


class StandInControls(torch.nn.Module):
    """stands in for Unit2Control inside the unmodified reference module: returns the drawn controls
    (ddsp/unit2control.py returns ``(controls dict, hidden)``)"""

    def __init__(self, ctrls):
        super().__init__()
        self.ctrls = ctrls

    def forward(self, units, f0, phase, volume, **kwargs):
        return self.ctrls, torch.zeros(units.shape[0], units.shape[1], 1)


def main():
    from make_golden import import_reference
    _, V = import_reference()
    import nsf_hifigan.nvSTFT as nv
    import torch.nn.functional as F
    W = basis()
    out = {}
    with mock.patch.object(nv, "librosa_mel_fn", side_effect=lambda **kw: W):
        stft = nv.STFT(SR, N_MELS, N_FFT, N_FFT, HOP, FMIN, FMAX)
        for tag in VJP_CASES:
            y, R = vjp_case(tag)
            y.requires_grad_(True)
            (stft.get_mel(y) * R).sum().backward()
            out["vjp_" + tag] = y.grad.numpy()
        for kind in CASCADE:
            f0, ctrls, draw, gt = cascade_inputs(kind)
            torch.manual_seed(0)
            model = (V.CombSubSuperFast(SR, HOP, N_FFT, n_unit=16, n_spk=1) if kind == "super"
                     else V.CombSubFast(SR, HOP, n_unit=16, n_spk=1))
            leaves = {k: v.clone().requires_grad_(True) for k, v in ctrls.items()}
            model.unit2ctrl = StandInControls(leaves)
            B, Fr = f0.shape[:2]
            name = "torch.randn_like" if kind == "super" else "torch.rand_like"
            with mock.patch(name, side_effect=lambda t: draw.to(t)):
                wav, _, _ = model(torch.zeros(B, Fr, 16), f0, torch.zeros(B, Fr, 1), infer=False)
            mel = stft.get_mel(wav).transpose(1, 2)
            assert mel.shape == gt.shape, (mel.shape, gt.shape)
            F.mse_loss(mel, gt).backward()
            for k, v in leaves.items():
                out[kind + "_grad_" + k] = v.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "mel_grad.npz"), **out)
    for k, v in out.items():
        print(k, v.shape, float(np.sqrt(np.mean(np.square(v.astype(np.float64))))))


if __name__ == "__main__":
    main()
