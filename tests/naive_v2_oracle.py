"""float64 numpy restatement of the layer of the reflow / diffusion-fast denoiser (``NaiveV2DiffLayer`` of the reference's
``reflow/naive_v2_diff.py``: no attention, not wavenet_like, a conv module without LayerNorm), for any D and Hc, in the layout
of the functional API (a frame's channels last):

    d   = Wp s + bp                         s [B, D], d [B, D]
    x'  = x + d + Wc cond + bc              x [B, L, D], cond [B, L, Hc]
    g   = glu(W1 x' + b1)                   rows [0, 2 D) times sigmoid(rows [2 D, 4 D))
    h   = silu(dw31(g) + bd)                a 31-tap cross-correlation per channel with 15 zeros on each side of g
    y   = x + W2 h + b2                     the residual is the x that came in

Deliberately wrong variants exist so that a test can show that its case tells them apart: ``leak_pad`` (x and cond are padded
with zeros instead of g, so the frames outside the sequence hold glu(W1 (d + bc) + b1)), ``residual_xp`` (the residual is x'),
``swap_glu`` (the halves of the GLU exchanged) and ``flip_taps`` (a convolution, not a correlation)."""
import numpy as np

TAPS = 31
PAD = TAPS // 2


def _sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def _f64(arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def xprime(x, cond, d, weights):
    wc, bc = _f64(weights[:2])
    x, cond, d = _f64((x, cond, d))
    return x + d[:, None, :] + cond @ wc[:, :, 0].T + bc


def pre_glu(x, cond, d, weights):
    """W1 x' + b1, [B, L, 4 D]: the first 2 D channels are the "out" half, the others the gate"""
    w1, b1 = _f64(weights[2:4])
    return xprime(x, cond, d, weights) @ w1[:, :, 0].T + b1


def _glu(z, swap=False):
    half = z.shape[-1] // 2
    out, gate = (z[..., half:], z[..., :half]) if swap else (z[..., :half], z[..., half:])
    return out * _sigmoid(gate)


def stencil(g, weights, flip_taps=False):
    """dw31(g) + bd over a g [B, L + 30, 2 D] that carries its padding"""
    wd, bd = _f64(weights[4:6])
    taps = wd[:, 0, ::-1] if flip_taps else wd[:, 0, :]
    L = g.shape[1] - 2 * PAD
    u = np.zeros((g.shape[0], L, g.shape[2])) + bd
    for j in range(TAPS):
        u = u + g[:, j:j + L, :] * taps[:, j]
    return u


def layer(x, cond, d, weights, leak_pad=False, residual_xp=False, swap_glu=False, flip_taps=False):
    """x [B, L, D], cond [B, L, Hc], d [B, D]; weights (wc [D, Hc, 1], bc, w1 [4 D, D, 1], b1, wd [2 D, 1, 31], bd,
    w2 [D, 2 D, 1], b2) -> y [B, L, D]"""
    w2, b2 = _f64(weights[6:8])
    x, cond, d = _f64((x, cond, d))
    pad = ((0, 0), (PAD, PAD), (0, 0))
    if leak_pad:
        g = _glu(pre_glu(np.pad(x, pad), np.pad(cond, pad), d, weights), swap_glu)
    else:
        g = np.pad(_glu(pre_glu(x, cond, d, weights), swap_glu), pad)
    u = stencil(g, weights, flip_taps)
    h = u * _sigmoid(u)
    res = xprime(x, cond, d, weights) if residual_xp else x
    return res + h @ w2[:, :, 0].T + b2


def project(s, proj):
    """d = Wp s + bp with wp [D, D, 1]"""
    wp, bp = _f64(proj)
    return np.asarray(s, np.float64) @ wp[:, :, 0].T + bp


def stack(x, cond, s, layers):
    """the layers of a denoiser: ``layers`` a list of (weights, (wp, bp)) -> x after the last layer"""
    x = np.asarray(x, np.float64)
    for weights, proj in layers:
        x = layer(x, cond, project(s, proj), weights)
    return x


def seeded_weights(D, Hc, seed, bias_std=0.1):
    """float32 ``(wc, bc, w1, b1, wd, bd, w2, b2)`` for unit-variance x and cond and a d of about 0.5: x' has a variance of about
    1.6, both halves in front of the GLU an rms of about 1 (the gate in its curved range), the stencil's output an rms of about 1
    and the branch W2 h + b2 the size of x (torch's default initialisation leaves the branch at a few per cent of x, and a dropped
    term would pass).  rms(g) is about 0.54 and rms(h) about 0.6 then."""
    rng = np.random.default_rng(seed)
    wc = rng.standard_normal((D, Hc, 1)) * (0.6 / np.sqrt(Hc))
    w1 = rng.standard_normal((4 * D, D, 1)) / np.sqrt(1.62 * D)
    wd = rng.standard_normal((2 * D, 1, TAPS)) / np.sqrt(TAPS * 0.293)
    w2 = rng.standard_normal((D, 2 * D, 1)) * (1.67 / np.sqrt(2 * D))
    bc, b1, bd, b2 = (bias_std * rng.standard_normal(n) for n in (D, 4 * D, 2 * D, D))
    return tuple(a.astype(np.float32) for a in (wc, bc, w1, b1, wd, bd, w2, b2))


def seeded_projection(D, seed):
    """float32 ``(wp [D, D, 1], bp [D])``: d = Wp s + bp of about 0.5 for a unit-variance s"""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((D, D, 1)) * (0.5 / np.sqrt(D))).astype(np.float32),
            (0.1 * rng.standard_normal(D)).astype(np.float32))


def load(layer, weights, proj=None):
    """copy ``seeded_weights`` (and a ``seeded_projection``) into a module with the layer's submodules: a stand-in or the
    reference's own class"""
    import torch
    net = layer.conformer.net
    with torch.no_grad():
        for p, a in zip((layer.condition_projection.weight, layer.condition_projection.bias, net[2].weight, net[2].bias,
                         net[4].weight, net[4].bias, net[6].weight, net[6].bias), weights):
            p.copy_(torch.as_tensor(a))
        if proj is not None:
            layer.diffusion_step_projection.weight.copy_(torch.as_tensor(proj[0]))
            layer.diffusion_step_projection.bias.copy_(torch.as_tensor(proj[1]))
    return layer
