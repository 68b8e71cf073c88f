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


# ---- exact restatements for tests/test_resample_edges.py -------------------------------------------------------------------------

TINY = float(np.finfo(np.float32).tiny)


def virt_group(n):
    """G of csrc/resample.h: the bank of n < 32 phases is expanded into 32 // n shifted copies"""
    return 32 // n if n < 32 else 1


def tap_index(o, n, w, T, p):
    """bank column that output t = q n + j holds against sample p: p + w - q o, for t < T -> (j [T], column [T])"""
    t = np.arange(T)
    return t % n, p + w - (t // n) * o


def impulse_readout(bank32, o, n, w, L, p, a):
    """x = 0 except x[p] = a (a power of two): y[q n + j] = a bank[j, p + w - q o] where that column is in [0, K), 0 elsewhere.
    One product per output, and scaling by a power of two is exact while nothing goes subnormal, so the float32 result is this
    in any summation order, fused or not -> float32 [T]"""
    assert 0 <= p < L and math.frexp(a)[0] in (0.5, -0.5), (p, L, a)
    K = bank32.shape[1]
    T = -(-n * L // o)
    j, col = tap_index(o, n, w, T, p)
    ok = (col >= 0) & (col < K)
    y = np.zeros(T, dtype=np.float64)
    y[ok] = a * bank32[j[ok], col[ok]].astype(np.float64)
    live = y != 0
    assert live.any() and np.abs(y[live]).min() >= TINY, "a product is subnormal: pick a larger a"
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    return y.astype(np.float32)


def reach(bank32, o, n, w, L, p):
    """which outputs sample p can reach -> (live [T], window [T]).  ``live``: the output's tap on the sample is not zero.
    ``window``: the output lies in a virtual row q' (G plain rows, n' = G n outputs) whose window of the padded input,
    [q' G o, q' G o + (G - 1) o + K), covers p + w -- the rows whose sums the kernel may put the sample into."""
    K = bank32.shape[1]
    T = -(-n * L // o)
    G = virt_group(n)
    j, col = tap_index(o, n, w, T, p)
    ok = (col >= 0) & (col < K)
    live = np.zeros(T, dtype=bool)
    live[ok] = bank32[j[ok], col[ok]] != 0
    qv = np.arange(T) // (G * n)
    d = p + w - qv * G * o
    window = (d >= 0) & (d < (G - 1) * o + K)
    assert not (live & ~window).any()
    return live, window


def exact_apply(x, o, n, bank32, w):
    """``apply`` for integer taps and samples: every partial sum is an integer below 2^24, so float32 holds it exactly in any
    order and the float64 sums are the answer bit for bit -> float32 [..., T]"""
    x = np.asarray(x)
    bound = float(np.abs(bank32).max()) * float(np.abs(x).max() if x.size else 0) * bank32.shape[1]
    assert np.array_equal(bank32, np.rint(bank32)) and np.array_equal(x, np.rint(x)) and bound < 2 ** 24, bound
    y = apply(x, o, n, bank32, w)
    assert np.abs(y).max(initial=0) < 2 ** 24
    return y.astype(np.float32)
