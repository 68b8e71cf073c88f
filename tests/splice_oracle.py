"""float64 numpy statement of the real-time caller's splice (gui.py:431-456) and of its ``phase_vocoder`` (gui.py:15-32), for the
tests of ddsp_svc_amd.splice.  Written from the contract (include/ddsp_hip.h), pinned to the reference's
own results by tests/golden/splice_*.npz.

Per utterance: seg = audio[L - (Bf + C + S + D) : L - D]; ratio[s] = sum_j seg[s + j] buf[j] / sqrt(sum_j seg[s + j]^2 + 1e-8)
(j < C, s = 0 .. S); shift = first argmax; tmp = seg[shift : shift + Bf + C]; its first C samples crossfaded with buf;
out = tmp[:Bf], new buffer = tmp[Bf:]."""
import numpy as np


def segment(audio, Bf, C, S, D):
    """the samples the splice looks at: audio[..., L - (Bf + C + S + D) : L - D]"""
    L = audio.shape[-1]
    return audio[..., L - (Bf + C + S + D): L - D]


def search_ratio(seg, buf, C, S):
    """nom[s] / den[s] for s = 0 .. S in float64 (one utterance)"""
    x = np.asarray(seg, np.float64)[: C + S]
    win = np.lib.stride_tricks.sliding_window_view(x, C)             # [S + 1, C]
    nom = win @ np.asarray(buf, np.float64)
    den = np.sqrt(np.sum(win * win, axis=1) + 1e-8)
    return nom / den


def near_tie(ratio, rel=1e-6):
    """True when the two best ratios are closer than ``rel`` of the best: either index is an honest argmax"""
    r = np.sort(np.asarray(ratio, np.float64))[::-1]
    return r.size > 1 and abs(r[0] - r[1]) <= rel * max(abs(r[0]), 1e-300)


def phase_vocoder(a, b, fade_out, fade_in, rows=256):
    """gui.py:15-32 in float64 with every phase argument reduced exactly: 2 pi (k t mod n) / n in integers, plus the bounded
    dphi_k t / n + phi_a,k.  Evaluated ``rows`` output samples at a time (n = 16384 would otherwise take 1 GB)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fo, fi = np.asarray(fade_out, np.float64), np.asarray(fade_in, np.float64)
    n = a.shape[0]
    w = np.sqrt(fo * fi)
    fa, fb = np.fft.rfft(a * w), np.fft.rfft(b * w)
    absab = np.abs(fa) + np.abs(fb)
    if n % 2 == 0:
        absab[1:-1] *= 2
    else:
        absab[1:] *= 2
    pa, pb = np.angle(fa), np.angle(fb)
    d = pb - pa
    d = d - 2 * np.pi * np.floor(d / 2 / np.pi + 0.5)
    k = np.arange(n // 2 + 1, dtype=np.int64)
    acc = np.empty(n)
    for t0 in range(0, n, rows):
        t = np.arange(t0, min(n, t0 + rows), dtype=np.int64)
        m = np.outer(t, k) % n
        arg = 2 * np.pi * m / n + (d[None, :] * t[:, None] / n + pa[None, :])
        acc[t0: t0 + t.size] = np.cos(arg) @ absab
    return a * fo ** 2 + b * fi ** 2 + acc * w / n


def splice(audio, buf, fade_in, fade_out, Bf, C, S, D, use_pv=False, shift=None, float32_crossfade=True):
    """One splice of every utterance of ``audio [B, L]`` with tails ``buf [B, C]`` -> (out [B, Bf], new_buf [B, C], shift [B],
    ratio [B, S + 1]).  ``shift`` given: use it instead of the argmax (a near tie the kernel resolved the other way).
    float32_crossfade: the plain crossfade as the torch chain rounds it, (x * fi) then + (buf * fo), in float32."""
    audio, buf = np.atleast_2d(audio), np.atleast_2d(buf)
    B = audio.shape[0]
    seg = segment(audio, Bf, C, S, D)
    outs, bufs, shifts, ratios = [], [], [], []
    for u in range(B):
        r = search_ratio(seg[u], buf[u], C, S)
        s = int(np.argmax(r)) if shift is None else int(np.atleast_1d(shift)[u])
        tmp = np.array(seg[u, s: s + Bf + C], np.float64)
        if use_pv:
            tmp[:C] = phase_vocoder(buf[u], tmp[:C], fade_out, fade_in)
        elif float32_crossfade:
            x, f_in, f_out = tmp[:C].astype(np.float32), np.asarray(fade_in, np.float32), np.asarray(fade_out, np.float32)
            tmp[:C] = (x * f_in) + (np.asarray(buf[u], np.float32) * f_out)
        else:
            tmp[:C] = tmp[:C] * np.asarray(fade_in, np.float64) + np.asarray(buf[u], np.float64) * np.asarray(fade_out, np.float64)
        outs.append(tmp[:Bf])
        bufs.append(tmp[Bf:])
        shifts.append(s)
        ratios.append(r)
    return np.stack(outs), np.stack(bufs), np.array(shifts, np.int64), np.stack(ratios)


def gui_windows(C):
    """fade_in / fade_out as gui.py:366-368 builds them (float32 arange of step 1 / C: it can hold C + 1 points, as torch's can)"""
    import torch
    fi = torch.sin(np.pi * torch.arange(0, 1, 1 / C) / 2) ** 2
    return fi.numpy(), (1 - fi).numpy()


def aten_phase_vocoder(old, new, f_out, f_in):
    """gui.py:15-32 as the ATen op sequence the GUI dispatches, in float32 with the GUI's own rounding (the ``[n, n/2 + 1]`` cosine
    argument reaches ~pi n radians, far beyond what float32 resolves); context for the tests and the torch side of
    tools/splice_latency.py, not a bar.  Ops in order: mul, sqrt; mul, rfft (twice); abs, abs, add; in-place mul of the inner
    bins; angle, angle, sub; div, div, add, floor, mul, sub (the wrap); arange, cast, mul, add; arange, unsqueeze, cast, div;
    mul, add, cos, mul, sum; pow, mul, pow, mul, add, mul, div, add."""
    import torch
    n = old.shape[0]
    taper = torch.sqrt(f_out * f_in)
    spec_old = torch.fft.rfft(old * taper)
    spec_new = torch.fft.rfft(new * taper)
    mag = torch.abs(spec_old) + torch.abs(spec_new)
    inner_end = n // 2 if n % 2 == 0 else n // 2 + 1          # the bins that stand for a conjugate pair
    mag[1:inner_end] *= 2
    ph_old = torch.angle(spec_old)
    dphi = torch.angle(spec_new) - ph_old
    dphi = dphi - (2 * np.pi) * torch.floor(dphi / 2 / np.pi + 0.5)
    omega = (2 * np.pi) * torch.arange(n // 2 + 1).to(old) + dphi
    frac = torch.arange(n).unsqueeze(-1).to(old) / n
    partials = torch.sum(mag * torch.cos(omega * frac + ph_old), -1)
    return old * f_out ** 2 + new * f_in ** 2 + partials * taper / n


class AtenSplice:
    """gui.py:431-456 as the ATen op sequence the GUI dispatches, with its state (the kept tail): two conv1d, pow, sqrt, div,
    argmax; a slice by a 0-dim device tensor (a device-to-host synchronisation); the crossfade (in-place mul and add) or
    ``aten_phase_vocoder``; the stereo repeat and the copy to the host into ``outdata [Bf, 2]``.  Returns the shift.  Like the
    GUI it edits ``audio`` in place and keeps its tail as a view into it."""

    def __init__(self, Bf, C, S, D, fade_in, fade_out, use_pv):
        import torch
        self.sizes, self.use_pv = (Bf, C, S, D), use_pv
        self.fade_in, self.fade_out = fade_in, fade_out
        self.tail = torch.zeros(C, device=fade_in.device)

    def __call__(self, audio, outdata):
        import torch
        import torch.nn.functional as F
        Bf, C, S, D = self.sizes
        region = audio[-(Bf + C + S + D): -D]
        probe = region[: C + S][None, None, :]
        corr = F.conv1d(probe, self.tail[None, None, :])
        energy = F.conv1d(probe ** 2, torch.ones(1, 1, C, device=audio.device))
        best = torch.argmax(corr[0, 0] / torch.sqrt(energy + 1e-8)[0, 0])
        picked = region[best: best + Bf + C]
        if self.use_pv:
            picked[:C] = aten_phase_vocoder(self.tail, picked[:C], self.fade_out, self.fade_in)
        else:
            picked[:C] *= self.fade_in
            picked[:C] += self.tail * self.fade_out
        self.tail = picked[-C:]
        outdata[:] = picked[:-C, None].repeat(1, 2).cpu().numpy()
        return int(best)


def wrap_margin(a, b, fade_out, fade_in):
    """distance of the vocoder's wrapped phase differences from +-pi over the complex bins (inputs closer than ~1e-4 are
    ill-conditioned: the float32 spectra of the device and the float64 ones of the oracle may wrap to opposite ends).  The real
    bins (DC, and Nyquist at even n) have angles of exactly 0 or pi on both sides and wrap alike."""
    w = np.sqrt(np.asarray(fade_out, np.float64) * np.asarray(fade_in, np.float64))
    fa, fb = np.fft.rfft(np.asarray(a, np.float64) * w), np.fft.rfft(np.asarray(b, np.float64) * w)
    d = np.angle(fb) - np.angle(fa)
    d = d - 2 * np.pi * np.floor(d / 2 / np.pi + 0.5)
    inner = d[1: (len(a) + 1) // 2]
    return float(np.min(np.pi - np.abs(inner))) if inner.size else np.pi
