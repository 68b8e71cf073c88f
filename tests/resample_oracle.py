"""float64 numpy restatement of torchaudio's sinc resampling (``_get_sinc_resample_kernel`` / ``_apply_sinc_resample_kernel``).

The bank follows torchaudio's op order: the phase offsets ``-j / n`` are a float32 quotient (torch evaluates int64 / int in the
default dtype), added to the float64 tap positions, and the bank is cast to float32.  The convolution with that float32 bank is
then summed in float64.
"""
import math

import numpy as np

KAISER_BETA = 14.769656459379492


def reduced(orig, new):
    g = math.gcd(int(orig), int(new))
    return int(orig) // g, int(new) // g


def bank(orig, new, lw=6, rolloff=0.99, method="sinc_interp_hann", beta=None):
    """-> (float32 [n, K] bank, width, float64 unclamped t of every tap)"""
    o, n = reduced(orig, new)
    base = min(o, n) * rolloff
    w = math.ceil(lw * o / base)
    idx = np.arange(-w, w + o, dtype=np.float64) / o
    q = np.array([np.float32(-j) / np.float32(n) for j in range(n)], dtype=np.float32).astype(np.float64)
    t_raw = (q[:, None] + idx[None, :]) * base
    t = np.clip(t_raw, -lw, lw)
    if method == "sinc_interp_hann":
        window = np.cos(t * math.pi / lw / 2) ** 2
    else:
        b32 = float(np.float32(KAISER_BETA if beta is None else beta))
        window = np.i0(b32 * np.sqrt(1 - (t / lw) ** 2)) / float(np.float32(np.i0(b32)))
    t = t * math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t)
    k = k * (window * (base / o))
    return k.astype(np.float32), w, t_raw


def apply(x, orig, new, bank32, w):
    """x [..., L] (any float dtype) -> float64 [..., ceil(n L / o)]"""
    o, n = reduced(orig, new)
    x = np.asarray(x, dtype=np.float64)
    shape = x.shape
    L = shape[-1]
    xs = x.reshape(int(np.prod(shape[:-1])), L)
    T = -(-n * L // o)
    K = bank32.shape[1]
    h = bank32.astype(np.float64)
    out = np.zeros((xs.shape[0], T))
    if T == 0:
        return out.reshape(shape[:-1] + (0,))
    M = -(-T // n)
    xp = np.zeros((xs.shape[0], (M - 1) * o + K))
    m = min(L, xp.shape[1] - w)
    xp[:, w:w + m] = xs[:, :m]
    idx = np.arange(M)[:, None] * o + np.arange(K)[None, :]            # [M, K]
    for b in range(xs.shape[0]):
        y = xp[b][idx] @ h.T                                            # [M, n]
        out[b] = y.reshape(-1)[:T]
    return out.reshape(shape[:-1] + (T,))


def resample(x, orig, new, lw=6, rolloff=0.99, method="sinc_interp_hann", beta=None):
    k, w, _ = bank(orig, new, lw, rolloff, method, beta)
    return apply(x, orig, new, k, w)
