"""float64 numpy restatement of the residual layer of the diffusion denoiser's WaveNet (``ResidualBlock`` of the reference's
``diffusion/wavenet.py``, dilation 1), for any C and H:

    d     = Wp s + bp                                  s [B, C], d [B, C]
    z     = dil3(x + d) + bdil + Wc cond + bc          x [B, C, T], cond [B, H, T], z [B, 2 C, T]
    g     = sigmoid(z[:C]) * tanh(z[C:])
    o     = Wo g + bo
    x_out = (x + o[:C]) / sqrt(2);  skip = o[C:]

dil3: a 3-tap cross-correlation with one zero on each side of ITS input x + d.  Deliberately wrong variants exist so that a test
can show that its case tells them apart: ``pad_with_d`` (zero-pads x, so the frames outside the sequence hold d), ``swap_gate``
(the halves of z exchanged), ``swap_out`` (the halves of o exchanged) and ``flip_taps`` (a convolution, not a correlation)."""
import numpy as np


def _sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def z_of(x, cond, d, weights, pad_with_d=False, flip_taps=False):
    wdil, bdil, wc, bc = [np.asarray(a, np.float64) for a in weights[:4]]
    x, cond, d = np.asarray(x, np.float64), np.asarray(cond, np.float64), np.asarray(d, np.float64)
    T = x.shape[2]
    if pad_with_d:
        y = np.pad(x, ((0, 0), (0, 0), (1, 1))) + d[:, :, None]
    else:
        y = np.pad(x + d[:, :, None], ((0, 0), (0, 0), (1, 1)))
    taps = wdil[:, :, ::-1] if flip_taps else wdil
    z = np.einsum("oh,bht->bot", wc[:, :, 0], cond) + (bdil + bc)[None, :, None]
    for j in range(3):
        z = z + np.einsum("oc,bct->bot", taps[:, :, j], y[:, :, j:j + T])
    return z


def layer(x, cond, d, weights, pad_with_d=False, swap_gate=False, swap_out=False, flip_taps=False):
    """x [B, C, T], cond [B, H, T], d [B, C]; weights (wdil [2 C, C, 3], bdil, wc [2 C, H, 1], bc, wo [2 C, C, 1], bo) ->
    (x_out, skip)"""
    wo, bo = np.asarray(weights[4], np.float64), np.asarray(weights[5], np.float64)
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    z = z_of(x, cond, d, weights, pad_with_d, flip_taps)
    gate, filt = (z[:, C:], z[:, :C]) if swap_gate else (z[:, :C], z[:, C:])
    g = _sigmoid(gate) * np.tanh(filt)
    o = np.einsum("oc,bct->bot", wo[:, :, 0], g) + bo[None, :, None]
    res, skip = (o[:, C:], o[:, :C]) if swap_out else (o[:, :C], o[:, C:])
    return (x + res) / np.sqrt(2.0), skip


def project(s, proj):
    """d = Wp s + bp"""
    wp, bp = np.asarray(proj[0], np.float64), np.asarray(proj[1], np.float64)
    return np.asarray(s, np.float64) @ wp.T + bp


def stack(x, cond, s, layers):
    """the residual layers of a WaveNet: ``layers`` a list of (weights, (wp, bp)) -> (x after the last layer, the sum of skips)"""
    x = np.asarray(x, np.float64)
    total = 0.0
    for weights, proj in layers:
        x, skip = layer(x, cond, project(s, proj), weights)
        total = total + skip
    return x, total


def seeded_weights(C, H, seed, bias_std=0.1):
    """float32 ``(wdil, bdil, wc, bc, wo, bo)`` for unit-variance x and cond and a d of about 0.5: rms(z) is about 1 (both
    non-linearities in their curved range) and the two halves of o are of x's size (torch's default initialisation leaves the
    residual at a few per cent of x, and a dropped term would pass).  rms(g) is about 0.31 at rms(z) = 1."""
    rng = np.random.default_rng(seed)
    wdil = rng.standard_normal((2 * C, C, 3)) * (0.75 / np.sqrt(3 * C * 1.25))
    wc = rng.standard_normal((2 * C, H, 1)) * (0.6 / np.sqrt(H))
    wo = rng.standard_normal((2 * C, C, 1)) * (3.2 / np.sqrt(C))
    bdil, bc, bo = (bias_std * rng.standard_normal(2 * C) for _ in range(3))
    return tuple(a.astype(np.float32) for a in (wdil, bdil, wc, bc, wo, bo))


def seeded_projection(C, seed):
    """float32 ``(wp [C, C], bp [C])``: d = Wp s + bp of about 0.5 for a unit-variance s"""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((C, C)) * (0.5 / np.sqrt(C))).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32))
