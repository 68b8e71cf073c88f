#!/usr/bin/env python
"""The NSF-HiFiGAN residual blocks on one MI355X: the HIP path (ddsp_svc_amd.nsf_generator) against the reference's op chain
under PyTorch-ROCm (F.leaky_relu / F.conv1d / add, as nsf_hifigan/models.py:61-68 and :253-259 run it) on the same GPU in the
same process, the two alternated rep by rep.

  --mode latency      B = 1, F = 203 frames (the GUI's 2.35 s window): the three stages the kernel covers (64 channels at 128 F
                      columns, 32 at 256 F, 16 at 512 F), a whole MRF stage (k = 3, 7, 11, dilations (1, 3, 5)) per call, and
                      each block (C, k) on its own for the dispatcher's crossover table.  Call to result: a host clock around
                      the call and a device synchronise.
  --mode throughput   B = 32 x 10 s (F = 861): the same, device events around each call.
  --stages wide       the two stages of the wide form (csrc/resblock_wide.h) instead: 256 channels at 8 F columns and 128 at
                      64 F, in the same two modes (default: narrow, the three stages above)

Every rep checks nothing; the first call of each pair is compared (max |hip - torch| relative to the output's RMS).  Prints
one JSON document; --out writes it to a file as well.
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

KS = (3, 7, 11)
DIL = (1, 3, 5)
STAGES = {"narrow": ((64, 128), (32, 256), (16, 512)),  # (channels, columns per frame)
          "wide": ((256, 8), (128, 64))}
PEAK_TFLOPS = 157.3                                     # f32 MFMA, MI355X


def weights(C, k, dev, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, std: (torch.randn(*s, generator=g) * std).to(dev)
    return [(mk(C, C, k, std=(C * k) ** -0.5), mk(C, std=0.1), mk(C, C, k, std=(C * k) ** -0.5), mk(C, std=0.1)) for _ in DIL]


def torch_block(x, ws):
    for (w1, b1, w2, b2), d in zip(ws, DIL):
        k = w1.shape[-1]
        xt = F.conv1d(F.leaky_relu(x, 0.1), w1, b1, dilation=d, padding=(k * d - d) // 2)
        xt = F.conv1d(F.leaky_relu(xt, 0.1), w2, b2, dilation=1, padding=(k - 1) // 2)
        x = xt + x
    return x


def torch_stage(x, blocks):
    xs = None
    for ws in blocks:
        if xs is None:
            xs = torch_block(x, ws)
        else:
            xs += torch_block(x, ws)
    return xs / len(blocks)


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


def compare(hip, ref, reps, warmup, events):
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
            "max_abs_diff_over_rms": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("latency", "throughput"), required=True)
    ap.add_argument("--stages", choices=tuple(STAGES), default="narrow")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resblock_bench: needs the GPU (no fallback)")
    from ddsp_svc_amd import nsf_generator as NG
    NG.TORCH_FASTER.clear()                            # measure the kernel everywhere, whatever the dispatcher would do
    dev = torch.device("cuda:0")
    lat = args.mode == "latency"
    B, frames = (1, 203) if lat else (32, 861)
    reps = args.reps or (40 if lat else 6)
    wide = args.stages == "wide"
    doc = {"mode": args.mode, "stage_set": args.stages, "B": B, "frames": frames, "reps": reps, "timing": "host clock + synchronise" if lat else "device events",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "stages": [], "blocks": []}
    with torch.no_grad():
        for C, per_frame in STAGES[args.stages]:
            T = per_frame * frames
            x = torch.randn(B, C, T, generator=torch.Generator().manual_seed(C)).to(dev)
            blocks = [weights(C, k, dev, 10 * C + k) for k in KS]
            specs = [(ws, DIL) for ws in blocks]
            r = compare(lambda: NG.mrf_stage(x, specs), lambda: torch_stage(x, blocks), reps, args.warmup, not lat)
            flops = sum(2.0 * 2 * len(DIL) * C * C * k for k in KS) * B * T
            r.update(C=C, T=T, launches_hip=(6 if wide else 3) * len(DIL), flops=flops, hip_tflops=flops / r["hip_ms"] * 1e-9,
                     hip_share_of_f32_mfma_peak=flops / r["hip_ms"] * 1e-9 / PEAK_TFLOPS)
            doc["stages"].append(r)
            print("stage", json.dumps(r), flush=True)
            for k, ws in zip(KS, blocks):
                rb = compare(lambda: NG.resblock1(x, ws, DIL), lambda: torch_block(x, ws), reps, args.warmup, not lat)
                fb = 2.0 * 2 * len(DIL) * C * C * k * B * T
                rb.update(C=C, k=k, T=T, hip_tflops=fb / rb["hip_ms"] * 1e-9, torch_tflops=fb / rb["torch_ms"] * 1e-9)
                doc["blocks"].append(rb)
                print("block", json.dumps(rb), flush=True)
            del x
            NG.release_workspace()
            torch.cuda.empty_cache()
    doc["torch_faster"] = [[b["C"], b["k"], b["T"]] for b in doc["blocks"] if b["torch_over_hip"] < 1.0]
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
