"""Shared by tests/test_parity_fast.py and tests/test_stft_tail_edges.py: seeded inputs of the short-time spectral filter
(``synth.stft_filter``, csrc/stft.hip), its windows, and its float64 reference written out on ``oracle.ddsp_oracle``."""
import numpy as np

from oracle import ddsp_oracle as O

HOP = 512


def hann(win):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)).astype(np.float32)


def asym_window(win, seed=7):
    """a positive window with no symmetry at all: a seeded draw from [0.25, 1.25) times a ramp from 0.5 to 1.5.  Under a Hann
    window w[i] == w[win - i], so a mirrored window index goes unseen; here it changes every sample."""
    rng = np.random.default_rng(seed)
    return ((0.25 + rng.random(win)) * np.linspace(0.5, 1.5, win)).astype(np.float32)


def _filter_case(B, F, win, seed, noise_phase=True, sigma_mag=1.0, sigma_phase=1.5):
    """exciter, noise [B, T] ~ N(0, 1); controls [B, F, win/2 + 1]: magnitudes ~ N(0, sigma_mag), phases ~ N(0, sigma_phase)"""
    rng = np.random.default_rng(seed)
    n = win // 2 + 1
    T = F * HOP
    exc = rng.standard_normal((B, T)).astype(np.float32)
    nz = rng.standard_normal((B, T)).astype(np.float32)
    hm, hp, nm, nph = [(s * rng.standard_normal((B, F, n))).astype(np.float32)
                       for s in (sigma_mag, sigma_phase, sigma_mag, sigma_phase)]
    return exc, nz, hm, hp, nm, (nph if noise_phase else None)


def _oracle_filter(exc, nz, hm, hp, nm, nph, win, w, reflect, normalize):
    Hs = O.spectral_filters(hm, hp)
    Hn = O.spectral_filters(nm, nph, 1.0 / 128.0)
    mode = "reflect" if reflect else "constant"
    w64 = w.astype(np.float64)
    spec = np.fft.rfft(O._frames(exc, win, HOP, mode) * w64, win) * Hs + \
        np.fft.rfft(O._frames(nz, win, HOP, mode) * w64, win) * Hn
    fr = np.fft.irfft(spec, win) * w64
    B, nfr, _ = fr.shape
    total = win + HOP * (nfr - 1)
    ola = np.zeros((B, total))
    env = np.zeros(total)
    for j in range(nfr):
        ola[:, j * HOP:j * HOP + win] += fr[:, j]
        env[j * HOP:j * HOP + win] += w64 * w64
    sl = slice(win // 2, win // 2 + HOP * (nfr - 1))
    return ola[:, sl] / env[sl] if normalize else ola[:, sl]
