#!/usr/bin/env python
"""The NSF-HiFiGAN generator's upsampling seams and output head on one MI355X: the HIP kernels (ddsp_svc_amd.nsf_generator:
upsample_stage, output_head) against the reference's op chain under PyTorch-ROCm (F.leaky_relu / F.conv_transpose1d / F.conv1d /
add, and F.leaky_relu / F.conv1d / torch.tanh, as nsf_hifigan/models.py:249-252 and :260-262 run them) on the same GPU in the
same process, the two alternated rep by rep.

  --mode latency      B = 1, F = 203 frames (the GUI's 2.35 s window): the three seams of the stock generator (128 -> 64 at 64 F
                      input columns, 64 -> 32 at 128 F, 32 -> 16 at 256 F; noise strides 4, 2, 1) and the head (16 channels at
                      512 F).  Call to result: a host clock around the call and a device synchronise.
  --mode throughput   B = 32 x 10 s (F = 861): the same, device events around each call.

Each entry carries the algorithmic bytes -- 4 (Cin Tin + Cout Tout + L) per utterance for a seam, 4 (C + 1) T for the head -- and
the share of the 8 TB/s roof they reach.  The first call of each pair is compared (max |hip - torch| relative to the output's
RMS).  Prints one JSON document; --out writes it to a file as well.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
import torch.nn.functional as F

SEAMS = ((64, 2, 4, 64), (32, 2, 2, 128), (16, 2, 1, 256))   # (Cout, u, s, input columns per frame)
HEAD = (16, 512)
HBM_BYTES_PER_S = 8e12


def timed(fn, events):
    if events:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def compare(hip, ref, reps, warmup, events, nbytes):
    """alternated: hip, torch, hip, torch, ...; median and spread of each, and the first results' difference"""
    yh, yt = hip(), ref()
    torch.cuda.synchronize()
    diff = float((yh - yt).abs().max() / yt.pow(2).mean().sqrt())
    del yh, yt
    for _ in range(warmup):
        hip()
        ref()
    torch.cuda.synchronize()
    th, tt = [], []
    for _ in range(reps):
        th.append(timed(hip, events))
        tt.append(timed(ref, events))
    q = lambda v: [float(np.percentile(v, p)) * 1e3 for p in (50, 10, 90)]
    (hm, hl, hh), (tm, tl, th_) = q(th), q(tt)
    return {"hip_ms": hm, "hip_ms_p10_p90": [hl, hh], "torch_ms": tm, "torch_ms_p10_p90": [tl, th_], "torch_over_hip": tm / hm,
            "max_abs_diff_over_rms": diff, "algorithmic_bytes": nbytes,
            "hip_fraction_of_hbm_roof": nbytes / (hm * 1e-3) / HBM_BYTES_PER_S,
            "torch_fraction_of_hbm_roof": nbytes / (tm * 1e-3) / HBM_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("latency", "throughput"), required=True)
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("generator_tail_bench: needs the GPU (no fallback)")
    from ddsp_svc_amd import nsf_generator as NG
    NG.SEAM_TORCH_FASTER.clear()                       # measure the kernels everywhere, whatever the dispatcher would do
    NG.HEAD_TORCH_FASTER.clear()
    dev = torch.device("cuda:0")
    lat = args.mode == "latency"
    B, frames = (1, 203) if lat else (32, 861)
    reps = args.reps or (40 if lat else 6)
    doc = {"mode": args.mode, "B": B, "frames": frames, "reps": reps, "timing": "host clock + synchronise" if lat else "device events",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "seams": [], "head": None}
    g = torch.Generator().manual_seed(1)
    mk = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(dev)
    with torch.no_grad():
        for Cout, u, s, per_frame in SEAMS:
            Cin, Tin, ks = 2 * Cout, per_frame * frames, (2 * s if s > 1 else 1)
            Tout, L = u * Tin, s * u * Tin
            x, src = mk(B, Cin, Tin), mk(B, 1, L)
            wu, bu, wn, bn = mk(Cin, Cout, 2 * u, std=(2 * Cin) ** -0.5), mk(Cout, std=0.1), mk(Cout, 1, ks, std=ks ** -0.5), mk(Cout, std=0.1)
            ref = lambda: (F.conv_transpose1d(F.leaky_relu(x, 0.1), wu, bu, stride=u, padding=u // 2)
                           + F.conv1d(src, wn, bn, stride=s, padding=s // 2 if s > 1 else 0))
            r = compare(lambda: NG.upsample_stage(x, wu, bu, u, src, wn, bn, s), ref, reps, args.warmup, not lat,
                        4.0 * B * (Cin * Tin + Cout * Tout + L))
            r.update(Cout=Cout, u=u, s=s, Tin=Tin, flops=2.0 * 2 * Cin * Cout * B * Tout)
            doc["seams"].append(r)
            print("seam", json.dumps(r), flush=True)
            del x, src
            torch.cuda.empty_cache()
        C, per_frame = HEAD
        T = per_frame * frames
        x, wp, bp = mk(B, C, T), mk(1, C, 7, std=(7 * C) ** -0.5), mk(1, std=0.1)
        r = compare(lambda: NG.output_head(x, wp, bp), lambda: torch.tanh(F.conv1d(F.leaky_relu(x), wp, bp, padding=3)), reps,
                    args.warmup, not lat, 4.0 * B * (C + 1) * T)
        r.update(C=C, T=T)
        doc["head"] = r
        print("head", json.dumps(r), flush=True)
    doc["torch_faster"] = {"seams": [[r["Cout"], r["u"], r["Tin"]] for r in doc["seams"] if r["torch_over_hip"] < 1.0],
                           "head": [[C, T]] if doc["head"]["torch_over_hip"] < 1.0 else []}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
