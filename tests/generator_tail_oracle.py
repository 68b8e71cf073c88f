"""float64 numpy restatement of the NSF-HiFiGAN generator's upsampling seam (nsf_hifigan/models.py:249-252) and output head
(:260-262), written from their two formulas:

    y[b, co, t] = bu[co] + sum over (ci, j) of lrelu_0.1(x)[b, ci, q] Wu[ci, co, j]      over t = u q - p + j,  k = 2 u, p = u / 2
                + bn[co] + sum over m of src[b, t s - s // 2 + m] Wn[co, 0, m]           2 s taps (s = 1: one tap, no padding)
    y[b, 0, t]  = tanh(bp + sum over (ci, j < 7) of lrelu_slope(x)[b, ci, t + j - 3] Wp[0, ci, j])

Both convolutions read zeros outside their input.  The keyword arguments produce the WRONG variants a kernel could compute
instead; the tests show that each of them differs from the right one by far more than the parity bar.
"""
import numpy as np

SLOPE = float(np.float32(0.1))                         # the float32 slopes the float32 code multiplies by
HEAD_SLOPE = float(np.float32(0.01))


def lrelu(v, slope=SLOPE):
    return np.where(v > 0, v, v * slope)


def conv_transpose(x, w, b, u, swap_taps=False, weight_as_conv=False):
    """x [B, Ci, Tin], w [Ci, Co, 2 u] (ConvTranspose1d's order), padding u / 2 -> [B, Co, u Tin], by scattering every tap.
    ``swap_taps``: the two taps of every output phase exchanged; ``weight_as_conv``: the same memory read as [Co, Ci, k]"""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    B, Ci, Tin = x.shape
    Co, k = w.shape[1], w.shape[2]
    assert k == 2 * u and w.shape[0] == Ci
    if weight_as_conv:
        w = w.reshape(Co, Ci, k).transpose(1, 0, 2)
    if swap_taps:
        w = np.concatenate([w[:, :, u:], w[:, :, :u]], axis=2)
    p = u // 2
    full = np.zeros((B, Co, u * Tin + k))                # column c is t = c - p ... + p: t = u q - p + j -> c = u q + j
    for j in range(k):
        full[:, :, j:j + u * Tin:u] += np.einsum("co,bcq->boq", w[:, :, j], x)
    return full[:, :, p:p + u * Tin] + b[None, :, None]


def noise_conv(src, w, b, s, unpadded_left=False):
    """src [B, L], w [Co, 1, 2 s] or [Co, 1, 1] at s = 1 -> [B, Co, L / s].  ``unpadded_left``: the window starts at t s"""
    src, w, b = np.asarray(src, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    B, L = src.shape
    ks = w.shape[-1]
    assert ks == (2 * s if s > 1 else 1) and L % s == 0
    off = 0 if (unpadded_left or s == 1) else s // 2
    n = L // s
    sp = np.zeros((B, off + L + ks))
    sp[:, off:off + L] = src
    out = np.broadcast_to(b[None, :, None], (B, w.shape[0], n)).copy()
    for m in range(ks):
        out += w[None, :, 0, m, None] * sp[:, None, m:m + n * s:s]
    return out


def seam(x, wu, bu, u, src, wn, bn, s, swap_taps=False, weight_as_conv=False, unpadded_left=False, replicate_edges=False):
    """``replicate_edges``: the input column before the first and behind the last read as a copy of its neighbour instead of
    zero -- it changes the first and the last u / 2 output columns only, whose second tap falls outside the sequence"""
    src = np.asarray(src)
    src = src.reshape(src.shape[0], -1)
    xl = lrelu(np.asarray(x, np.float64))
    if replicate_edges:
        Tout = u * xl.shape[-1]
        xl = np.concatenate([xl[:, :, :1], xl, xl[:, :, -1:]], axis=2)
        up = conv_transpose(xl, wu, bu, u, swap_taps, weight_as_conv)[:, :, u:u + Tout]
    else:
        up = conv_transpose(xl, wu, bu, u, swap_taps, weight_as_conv)
    return up + noise_conv(src, wn, bn, s, unpadded_left)


def head(x, w, b, slope=HEAD_SLOPE):
    """x [B, C, T], w [1, C, 7], b [1] -> [B, 1, T]"""
    x, w, b = lrelu(np.asarray(x, np.float64), slope), np.asarray(w, np.float64), np.asarray(b, np.float64)
    B, C, T = x.shape
    xp = np.zeros((B, C, T + 6))
    xp[:, :, 3:3 + T] = x
    out = np.full((B, 1, T), b[0])
    for j in range(7):
        out[:, 0] += np.einsum("c,bct->bt", w[0, :, j], xp[:, :, j:j + T])
    return np.tanh(out)


def seeded_seam_weights(Cout, u, s, seed, bias_std=0.1):
    """float32 (wu, bu, wn, bn): weights at std 1 / sqrt(fan-in) -- 2 Cin products per output for the transposed convolution,
    its 2 s (or 1) taps for the noise convolution -- and biases at ``bias_std``"""
    rng = np.random.default_rng(seed)
    Cin, ks = 2 * Cout, (2 * s if s > 1 else 1)
    return tuple(a.astype(np.float32) for a in (
        rng.standard_normal((Cin, Cout, 2 * u)) / np.sqrt(2 * Cin), rng.standard_normal(Cout) * bias_std,
        rng.standard_normal((Cout, 1, ks)) / np.sqrt(ks), rng.standard_normal(Cout) * bias_std))


def seeded_head_weights(C, seed, bias_std=0.1):
    rng = np.random.default_rng(seed)
    return tuple(a.astype(np.float32) for a in (rng.standard_normal((1, C, 7)) / np.sqrt(7 * C), rng.standard_normal(1) * bias_std))
