"""A float64 numpy statement of the performer's softmax-kernel linear attention, written from the mathematics and generic in the
head width d, the feature count m and the head count H; and the seeded inputs the attention tests share.

Per batch item and head, q, k, v [N, d], the projection P [m, d], dn = d^-0.25, ratio = m^-0.5:

    (normalize)  q = q / (|q| + 1e-8),  k = k / (|k| + 1e-8)
    dq = (dn q) P^T,  dk = (dn k) P^T;   gq = |q|^2 / 2 * dn^2,  gk = |k|^2 / 2 * dn^2
    q' = ratio (exp(dq - gq - rowmax(dq)) + 1e-4);   k' = ratio exp(dk - gk + 1e-4)
    out = (q' (k'^T v)) / (q' . sum_n k' + 1e-8)
"""
import numpy as np


def feature_map(x, proj, is_query):
    x = np.asarray(x, np.float64)
    proj = np.asarray(proj, np.float64)
    d, m = x.shape[-1], proj.shape[0]
    dn, ratio = d ** -0.25, m ** -0.5
    dash = (dn * x) @ proj.T
    g = (x * x).sum(-1, keepdims=True) / 2.0 * dn * dn
    if is_query:
        return ratio * (np.exp(dash - g - dash.max(-1, keepdims=True)) + 1e-4)
    return ratio * np.exp(dash - g + 1e-4)


def fast_attention(q, k, v, proj, normalize=False):
    """q, k, v [..., N, d] -> [..., N, d] in float64"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    if normalize:
        q = q / (np.sqrt((q * q).sum(-1, keepdims=True)) + 1e-8)
        k = k / (np.sqrt((k * k).sum(-1, keepdims=True)) + 1e-8)
    qp, kp = feature_map(q, proj, True), feature_map(k, proj, False)
    ksum = kp.sum(-2)                                  # [..., m]
    ctx = np.swapaxes(kp, -1, -2) @ v                  # [..., m, d]
    den = (qp * ksum[..., None, :]).sum(-1, keepdims=True) + 1e-8
    return (qp @ ctx) / den


def self_attention(x, w, proj, heads, normalize=False):
    """x [B, N, D], w = (wq, bq, wk, bk, wv, bv, wo, bo) with the Linear layers' [out, in] weights -> [B, N, Dout] in float64"""
    x = np.asarray(x, np.float64)
    wq, bq, wk, bk, wv, bv, wo, bo = (np.asarray(a, np.float64) for a in w)
    B, N, _ = x.shape

    def split(t):
        return t.reshape(B, N, heads, -1).transpose(0, 2, 1, 3)

    q, k, v = split(x @ wq.T + bq), split(x @ wk.T + bk), split(x @ wv.T + bv)
    o = fast_attention(q, k, v, proj, normalize)
    return o.transpose(0, 2, 1, 3).reshape(B, N, -1) @ wo.T + bo


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------

def seeded_projection(d, m, seed):
    """rows of about the length sqrt(d), as ``gaussian_orthogonal_random_matrix`` draws them with scaling 0"""
    return np.random.default_rng(seed).standard_normal((m, d)).astype(np.float32)


def seeded_qkv(B, H, N, d, seed, scale=1.0):
    """q and k at ``scale`` sigma, v at 1 sigma; every (b, h) gets its own data"""
    rng = np.random.default_rng(seed)
    q = (scale * rng.standard_normal((B, H, N, d))).astype(np.float32)
    k = (scale * rng.standard_normal((B, H, N, d))).astype(np.float32)
    v = rng.standard_normal((B, H, N, d)).astype(np.float32)
    return q, k, v


def seeded_linear(D, heads, d, seed, dout=None):
    """(wq, bq, wk, bk, wv, bv, wo, bo): q, k, v of about 1 sigma for x of 1 sigma"""
    rng = np.random.default_rng(seed)
    inner, dout = heads * d, D if dout is None else dout
    w = []
    for _ in range(3):
        w += [(rng.standard_normal((inner, D)) / np.sqrt(D)).astype(np.float32), (0.1 * rng.standard_normal(inner)).astype(np.float32)]
    w += [(rng.standard_normal((dout, inner)) / np.sqrt(inner)).astype(np.float32), (0.1 * rng.standard_normal(dout)).astype(np.float32)]
    return tuple(w)
