"""float64 numpy statement of the frame features of the real-time path, for the tests of ddsp_svc_amd.features: the volume envelope
(ddsp/vocoder.py:147-157), the silence mask and gate (gui.py:114-118, :134), the salience decode (encoder/rmvpe/utils.py:106-121),
the F0 track (ddsp/vocoder.py:104-105, :110-118, :139-143) and the pools (ddsp/core.py:8-45).  Written from the contract
(include/ddsp_hip.h) with the reference's dtype flow -- the float32 comparisons, the float32 store of the first fill, float64
``np.interp`` -- and pinned to the reference's own results by tests/golden/features_*.npz (make_golden_features.py).

Also here: ``Aten*``, the same mathematics as torch ops on one device, which tools/features_latency.py times the kernels against."""
import numpy as np

N_CLASS, CENTS_BASE = 360, 1997.3794084376191


# ---- volume -----------------------------------------------------------------------------------------------------------------
def volume(audio, hop):
    """[T] or [B, T] float32 -> float64 [.., T // hop + 1]: the exact squares, float64 means"""
    a = np.atleast_2d(np.asarray(audio, np.float32)).astype(np.float64)
    T = a.shape[1]
    F = T // hop + 1
    a2 = np.pad(a * a, ((0, 0), (hop // 2, (hop + 1) // 2)), mode="reflect")
    v = np.sqrt(a2[:, : F * hop].reshape(a.shape[0], F, hop).mean(axis=2))
    return v[0] if np.ndim(audio) == 1 else v


# ---- mask and gate ----------------------------------------------------------------------------------------------------------
def threshold(db):
    return np.float32(10 ** (float(db) / 20))


def frame_mask(vol, db, dilate=4):
    """gui.py:114-116 on float32 volumes [F] or [B, F] -> float64 zeros and ones"""
    v = np.atleast_2d(np.asarray(vol, np.float32))
    m = (v > threshold(db)).astype(np.float64)
    m = np.pad(m, ((0, 0), (dilate, dilate)), mode="edge")
    m = np.stack([m[:, n: n + 2 * dilate + 1].max(axis=1) for n in range(v.shape[1])], axis=1)
    return m[0] if np.ndim(vol) == 1 else m


def upsample(mask, block):
    """ddsp/core.py upsample on [.., F]: linear between consecutive frames, the last frame held -> float64 [.., F block]"""
    m = np.asarray(mask, np.float64)
    nxt = np.concatenate([m[..., 1:], m[..., -1:]], axis=-1)
    r = np.arange(block, dtype=np.float64) / block
    return (m[..., None] + (nxt - m)[..., None] * r).reshape(m.shape[:-1] + (m.shape[-1] * block,))


def upsample_torch_f32(mask, block):
    """the float32 arithmetic of ``F.interpolate(mode='linear', align_corners=True)`` as ``upsample`` calls it: the source
    position scale * i with scale = float32(F) / float32(F block), weights (1 - lambda, lambda)"""
    m = np.concatenate([np.asarray(mask, np.float32), np.asarray(mask, np.float32)[-1:]])
    F = m.shape[0] - 1
    scale = np.float32(F) / np.float32(F * block)
    src = scale * np.arange(F * block, dtype=np.float32)
    i0 = np.minimum(src.astype(np.int64), F)
    i1 = np.minimum(i0 + 1, F)
    l1 = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1))
    return (np.float32(1) - l1) * m[i0] + l1 * m[i1]


def volume_margin(vol, db):
    """the smallest relative distance of a volume from the threshold"""
    t = float(threshold(db))
    return float(np.min(np.abs(np.asarray(vol, np.float64) - t)) / t)


# ---- salience decode ----------------------------------------------------------------------------------------------------------
def decode_salience(hidden, thred=0.03, center=None):
    """[B, N, 360] float32 -> float64 [B, N]"""
    h32 = np.asarray(hidden, np.float32)
    h = h32.astype(np.float64)
    idx = np.arange(N_CLASS)[None, None, :]
    c = np.argmax(h32, axis=2)[..., None] if center is None else np.asarray(center, np.int64).reshape(h.shape[:2] + (1,))
    w = h * ((idx >= np.clip(c - 4, 0, None)) & (idx < np.clip(c + 5, None, N_CLASS)))
    ps, ws = np.sum(w * (idx * 20.0 + CENTS_BASE), axis=2), np.sum(w, axis=2)
    f0 = 10.0 * 2.0 ** (ps / (ws + (ws == 0)) / 1200.0)
    return f0 * ~(h32.max(axis=2) < np.float32(thred))


# ---- F0 track -----------------------------------------------------------------------------------------------------------------
def _fill(f0):
    uv = f0 == 0
    if len(f0[~uv]) > 0:
        f0[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], f0[~uv])     # stored in f0's own dtype
    return uv


def retimed_uv(f0_src, src_period, hop, sr, n):
    """the retimed unvoiced flag of the linear mode, float64 [n] (the tests keep it away from 0.5)"""
    f0 = np.asarray(f0_src, np.float32)
    return np.interp(hop / sr * np.arange(n), src_period * np.arange(len(f0)), (f0 == 0).astype(float))


def f0_track(f0_src, src_period, hop, sr, n_frames, start_frame=0, mode="linear", uv_interp=False, f0_min=65.0):
    """one row [N] float32 -> float64 [n_frames], the statements of ddsp/vocoder.py in their order"""
    f0 = np.array(f0_src, np.float32)
    n = n_frames - start_frame
    if mode == "linear":
        uv = _fill(f0)                                                                    # float32 store
        origin = src_period * np.arange(len(f0))
        target = hop / sr * np.arange(n)
        out = np.interp(target, origin, f0)
        out[np.interp(target, origin, uv.astype(float)) > 0.5] = 0
    else:
        out = np.array([f0[int(min(int(np.round(k * hop / sr / src_period)), len(f0) - 1))] for k in range(n)], np.float64)
    out = np.pad(out, (start_frame, 0))
    if uv_interp:
        _fill(out)
        out[out < f0_min] = f0_min
    return out


# ---- pools --------------------------------------------------------------------------------------------------------------------
def _windows(x, k):
    xp = np.pad(np.asarray(x, np.float32), ((0, 0), ((k - 1) // 2, k // 2)), mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(xp, k, axis=1)                       # [B, N, k]


def masked_avg_pool(x, k):
    """float32 [B, N] -> the float32 restatement: a float64 sum of the values that are not NaN over max(count, 1), rounded once"""
    w = _windows(x, k).astype(np.float64)
    ok = ~np.isnan(w)
    return (np.where(ok, w, 0.0).sum(axis=2) / np.maximum(ok.sum(axis=2), 1)).astype(np.float32)


def median_pool(x, k):
    return np.sort(_windows(x, k), axis=2)[:, :, (k - 1) // 2]                           # NaN last, as torch.sort


# ---- helpers for the assertions ---------------------------------------------------------------------------------------------
def ulp_diff(got, want):
    """|got - float32(want)| in units of float32(want)'s ulp"""
    w = np.asarray(want, np.float64).astype(np.float32)
    return np.abs(np.asarray(got, np.float64) - w.astype(np.float64)) / np.spacing(np.maximum(np.abs(w), np.float32(1e-30))).astype(np.float64)


# ---- the same mathematics as torch ops on one device (the yardstick of tools/features_latency.py) ----------------------------
def aten_volume(audio, hop):
    """[B, T] -> [B, F]: square, reflect pad, mean over hops, sqrt"""
    import torch
    import torch.nn.functional as F
    B, T = audio.shape
    n = T // hop + 1
    a2 = F.pad((audio * audio).unsqueeze(1), (hop // 2, (hop + 1) // 2), mode="reflect").squeeze(1)
    return a2[:, : n * hop].reshape(B, n, hop).mean(dim=2).sqrt()


def aten_mask(volume, db, block, dilate=4):
    """[B, F] -> the upsampled [B, F block] mask: threshold, replicate pad, max pool, linear interpolation"""
    import torch
    import torch.nn.functional as F
    m = (volume > float(threshold(db))).float().unsqueeze(1)
    m = F.max_pool1d(F.pad(m, (dilate, dilate), mode="replicate"), 2 * dilate + 1, stride=1)
    m = torch.cat((m, m[:, :, -1:]), 2)
    return F.interpolate(m, size=(m.shape[-1] - 1) * block + 1, mode="linear", align_corners=True)[:, 0, :-1]


def aten_gate(signal, volume, db, block, dilate=4):
    return signal * aten_mask(volume, db, block, dilate)


def aten_decode(hidden, thred=0.03):
    """to_local_average_f0 op for op, without the transfer to the host"""
    import torch
    idx = torch.arange(N_CLASS, device=hidden.device)[None, None, :]
    idx_cents = idx * 20 + CENTS_BASE
    center = torch.argmax(hidden, dim=2, keepdim=True)
    start = torch.clip(center - 4, min=0)
    end = torch.clip(center + 5, max=N_CLASS)
    weights = hidden * ((idx >= start) & (idx < end))
    product_sum = torch.sum(weights * idx_cents, dim=2)
    weight_sum = torch.sum(weights, dim=2)
    cents = product_sum / (weight_sum + (weight_sum == 0))
    f0 = 10 * 2 ** (cents / 1200)
    return f0 * ~(hidden.max(dim=2)[0] < thred)


def _aten_fill(f0):
    """[B, N] -> zeros filled between the nearest nonzero neighbours, edges held (rows without one unchanged)"""
    import torch
    B, N = f0.shape
    i = torch.arange(N, device=f0.device).expand(B, N)
    voiced = f0 != 0
    p = torch.cummax(torch.where(voiced, i, torch.full_like(i, -1)), dim=1)[0]
    q = torch.flip(torch.cummin(torch.flip(torch.where(voiced, i, torch.full_like(i, N)), [1]), dim=1)[0], [1])
    fp, fq = torch.gather(f0, 1, p.clamp(min=0)), torch.gather(f0, 1, q.clamp(max=N - 1))
    w = (i - p).to(f0.dtype) / (q - p).clamp(min=1).to(f0.dtype)
    mid = fp + (fq - fp) * w
    out = torch.where(p < 0, fq, torch.where(q >= N, fp, mid))
    return torch.where((p < 0) & (q >= N), f0, out)


def aten_track(f0_src, src_period, hop, sr, n_frames, uv_interp=True, f0_min=65.0):
    """the linear mode of the track as torch ops in float64 on the device ([B, N] -> [B, n_frames])"""
    import torch
    f = _aten_fill(f0_src).double()
    u = (f0_src == 0).double()
    N = f.shape[1]
    x = hop / sr * torch.arange(n_frames, device=f.device, dtype=torch.float64)
    j = torch.clamp((x / src_period).floor().long(), max=N - 1)
    j1 = torch.clamp(j + 1, max=N - 1)
    w = ((x - src_period * j) / src_period).clamp(0, 1)

    def lerp(v):
        a, b = v[:, j], v[:, j1]
        return a + (b - a) * w
    out = torch.where(lerp(u) > 0.5, torch.zeros_like(x), lerp(f))
    if uv_interp:
        out = _aten_fill(out).clamp(min=f0_min)
    return out.float()
