"""float64 numpy restatement of the conformer conv module (``ConformerConvModule`` of the reference's
``model_conformer_naive.py`` and ``ddsp/pcmer.py``), for any D:

    net(x) = W2 silu(dw(glu(W1 ln(x) + b1)) + bd) + b2                    x [B, L, D]

ln: optional LayerNorm over D (biased variance); glu: rows [0, 2 D) times sigmoid of rows [2 D, 4 D); dw: a k-tap
cross-correlation per channel with (k - 1) / 2 zeros on each side of ITS input.  Three deliberately wrong variants exist so that a
test can show that its case tells them apart: ``halo_from_padded_x`` (zero-pads x instead of the GLU's output, so the frames
outside the sequence hold glu(b1)), ``swap_glu`` (the halves exchanged) and ``flip_taps`` (a convolution, not a correlation)."""
import numpy as np


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def layer_norm(x, gamma, beta, eps):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * gamma + beta


def net(x, weights, norm=None, eps=1e-5, halo_from_padded_x=False, swap_glu=False, flip_taps=False):
    """x [B, L, D]; weights (w1 [4 D, D, 1], b1, wd [2 D, 1, k], bd, w2 [D, 2 D, 1], b2); norm (gamma, beta) or None"""
    w1, b1, wd, bd, w2, b2 = [np.asarray(a, np.float64) for a in weights]
    x = np.asarray(x, np.float64)
    B, L, D = x.shape
    k = wd.shape[-1]
    h = (k - 1) // 2
    I = wd.shape[0]
    if norm is not None:
        x = layer_norm(x, np.asarray(norm[0], np.float64), np.asarray(norm[1], np.float64), eps)
    if halo_from_padded_x:
        x = np.pad(x, ((0, 0), (h, h), (0, 0)))
    u = x @ w1[:, :, 0].T + b1                         # [B, L (+ 2 h), 4 D]
    out, gate = (u[..., I:], u[..., :I]) if swap_glu else (u[..., :I], u[..., I:])
    g = out * _sigmoid(gate)
    if not halo_from_padded_x:
        g = np.pad(g, ((0, 0), (h, h), (0, 0)))
    taps = wd[:, 0, ::-1] if flip_taps else wd[:, 0, :]
    s = np.zeros((B, L, I))
    for j in range(k):
        s += g[:, j:j + L, :] * taps[:, j]
    s += bd
    s = s * _sigmoid(s)
    return s @ w2[:, :, 0].T + b2


def encoder(x, layers):
    """x = x + net_i(x) over ``layers``, a list of (weights, norm, eps)"""
    x = np.asarray(x, np.float64)
    for weights, norm, eps in layers:
        x = x + net(x, weights, norm, eps)
    return x


def seeded_weights(D, seed, bias_std=0.1, k=31, asymmetric=False):
    """float32 weights scaled so that rms(net(x)) is of the size of a unit-variance x (torch's default initialisation gives 0.06,
    and a test on that would mostly test the residual add).  ``asymmetric``: taps that grow along j, so a flip shows."""
    rng = np.random.default_rng(seed)
    I = 2 * D
    w1 = rng.standard_normal((2 * I, D, 1)) * (1.6 / np.sqrt(D))
    wd = rng.standard_normal((I, 1, k)) * (1.8 / np.sqrt(k))
    if asymmetric:
        wd = wd * np.linspace(0.2, 1.8, k)
    w2 = rng.standard_normal((D, I, 1)) * (1.0 / np.sqrt(I))
    b1, bd, b2 = (bias_std * rng.standard_normal(n) for n in (2 * I, I, D))
    return tuple(a.astype(np.float32) for a in (w1, b1, wd, bd, w2, b2))


def seeded_norm(D, seed):
    rng = np.random.default_rng(seed)
    return (1.0 + 0.3 * rng.standard_normal(D)).astype(np.float32), (0.2 * rng.standard_normal(D)).astype(np.float32)
