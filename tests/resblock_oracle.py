"""float64 numpy restatement of the NSF-HiFiGAN residual block (nsf_hifigan/models.py:37-68 and :253-259), written from its
three formulas:

    xt = lrelu(x, 0.1); xt = conv1d(xt, w1, b1, dilation=d, padding=(k*d - d)//2)
    xt = lrelu(xt, 0.1); xt = conv1d(xt, w2, b2, dilation=1, padding=(k - 1)//2)
    y  = xt + x

Each conv zero-pads its own input.  ``halo_from_padded_x=True`` is the WRONG variant a tiled kernel produces when it computes
the intermediate beyond [0, T) from zero-padded x instead of zeroing it: the edge tests show that it differs.
"""
import numpy as np

SLOPE = float(np.float32(0.1))                         # the float32 slope the float32 code multiplies by


def lrelu(v):
    return np.where(v > 0, v, v * SLOPE)


def conv1d(x, w, b, d, pad):
    """x [B, C, T] zero-padded by ``pad`` on both sides, w [Co, Ci, k], b [Co], dilation d -> [B, Co, T + 2 pad - (k - 1) d]"""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    B, C, T = x.shape
    k = w.shape[-1]
    xp = np.zeros((B, C, T + 2 * pad))
    xp[:, :, pad:pad + T] = x
    n = T + 2 * pad - (k - 1) * d
    out = np.broadcast_to(b[None, :, None], (B, w.shape[0], n)).copy()
    for j in range(k):
        out += np.einsum("oc,bct->bot", w[:, :, j], xp[:, :, j * d:j * d + n])
    return out


def pair(x, w1, b1, w2, b2, d, halo_from_padded_x=False):
    x = np.asarray(x, np.float64)
    k = np.asarray(w1).shape[-1]
    h = (k - 1) // 2
    if halo_from_padded_x:
        xt = lrelu(conv1d(lrelu(x), w1, b1, d, h * d + h))       # the intermediate on [-h, T + h), none of it zeroed
        return conv1d(xt, w2, b2, 1, 0) + x
    xt = conv1d(lrelu(x), w1, b1, d, (k * d - d) // 2)
    return conv1d(lrelu(xt), w2, b2, 1, h) + x


def block(x, weights, dilations, halo_from_padded_x=False):
    """weights: one (w1, b1, w2, b2) per pair"""
    x = np.asarray(x, np.float64)
    for (w1, b1, w2, b2), d in zip(weights, dilations):
        x = pair(x, w1, b1, w2, b2, d, halo_from_padded_x)
    return x


def stage(x, blocks):
    """blocks: a list of (weights, dilations); the sum of the blocks' outputs divided by their number"""
    xs = None
    for weights, dilations in blocks:
        r = block(x, weights, dilations)
        xs = r if xs is None else xs + r
    return xs / len(blocks)


def seeded_weights(C, k, pairs, seed, bias_std=0.1):
    """float32 weights at std 1 / sqrt(C k) (so that a conv keeps the scale of its input) and biases at ``bias_std``"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(pairs):
        out.append(tuple(a.astype(np.float32) for a in (
            rng.standard_normal((C, C, k)) / np.sqrt(C * k), rng.standard_normal(C) * bias_std,
            rng.standard_normal((C, C, k)) / np.sqrt(C * k), rng.standard_normal(C) * bias_std)))
    return out
