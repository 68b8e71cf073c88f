#!/usr/bin/env python
"""The performer attention of PCmer (8 heads of 64, 266 features) on one MI355X: the HIP path (ddsp_svc_amd.attention) against the
same op chain as torch ops under PyTorch-ROCm (the reference's softmax_kernel / linear_attention / SelfAttention.forward, restated
here) on the same GPU in the same process with the same weights, the two alternated step by step.

  fast_attention   the FastAttention core on q, k, v [B, 8, N, 64]
  self_attention   one whole SelfAttention(256): three Linear layers (one addmm on the HIP side), the core, to_out

  throughput   both at B = 32 x 862 frames (10 s) and B = 48 x 172 (2 s training crops), device events around each call
               -> profiles/attention_throughput.json
  latency      both at B = 1 x 100 (the streaming shape) and B = 1 x 203 frames (the GUI's 2.35 s window), call to result: a
               host clock around the call and a device synchronise  -> profiles/attention_latency.json

Each pair runs --steps alternated steps and is timed over the LAST --tail of them.  The achieved fraction of the 155 TF f32 MFMA
peak is reported on the algorithmic flops, 2 x 266 x (3 x 64 + 65) per frame and head, and on the flops the two kernels execute
(17 feature fragments x 64 MFMAs of 16x16x4 per block of 16 frames and head); for self_attention both count the attention
kernels only, the time is the whole module's.  ``torch_faster_frames`` lists the B N at which torch was faster at the
fast_attention case: what ATTN_TORCH_FASTER is filled from.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

D, HEADS, DH, M = 256, 8, 64, 266
PEAK_TFLOPS = 155.0                                    # measured f32 MFMA peak of one MI355X
SHAPES = {"throughput": ((32, 862), (48, 172)), "latency": ((1, 100), (1, 203))}


def torch_feature_map(x, proj, is_query):
    dn, ratio = DH ** -0.25, M ** -0.5
    dash = torch.einsum("...id,...jd->...ij", dn * x, proj.expand(*x.shape[:2], *proj.shape))
    g = (x ** 2).sum(-1) / 2.0 * dn ** 2
    g = g.unsqueeze(-1)
    if is_query:
        return ratio * (torch.exp(dash - g - dash.max(-1, keepdim=True).values) + 1e-4)
    return ratio * torch.exp(dash - g + 1e-4)


def torch_fast(q, k, v, proj):
    q, k = torch_feature_map(q, proj, True), torch_feature_map(k, proj, False)
    ksum = k.sum(-2)
    dinv = 1.0 / (torch.einsum("...nd,...d->...n", q, ksum) + 1e-8)
    ctx = torch.einsum("...nd,...ne->...de", k, v)
    return torch.einsum("...de,...nd,...n->...ne", ctx, q, dinv)


def torch_self(x, w, proj):
    wq, bq, wk, bk, wv, bv, wo, bo = w
    B, N, _ = x.shape
    q, k, v = (F.linear(x, a, b).view(B, N, HEADS, DH).permute(0, 2, 1, 3) for a, b in ((wq, bq), (wk, bk), (wv, bv)))
    out = torch_fast(q, k, v, proj)
    return F.linear(out.permute(0, 2, 1, 3).reshape(B, N, HEADS * DH), wo, bo)


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


def compare(hip, ref, steps, tail, events):
    """alternated: hip, torch, hip, torch, ...; the median and spread of each over the last ``tail`` steps"""
    yh, yt = hip(), ref()
    torch.cuda.synchronize()
    diff = float((yh - yt).abs().max() / yt.pow(2).mean().sqrt())
    del yh, yt
    th, tt = [], []
    for _ in range(steps):
        th.append(timed(hip, events))
        tt.append(timed(ref, events))
    q = lambda v: [float(np.percentile(v[-tail:], p)) * 1e3 for p in (50, 10, 90)]
    (hm, hl, hh), (tm, tl, tu) = q(th), q(tt)
    return {"hip_ms": hm, "hip_ms_p10_p90": [hl, hh], "torch_ms": tm, "torch_ms_p10_p90": [tl, tu], "torch_over_hip": tm / hm,
            "hip_ms_first_steps": float(np.median(th[:10])) * 1e3, "max_abs_diff_over_rms": diff}


def flops(B, N):
    alg = 2.0 * M * (3 * DH + DH + 1) * B * HEADS * N
    exe = 2.0 * 16 * 16 * 4 * 17 * 64 * -(-N // 16) * B * HEADS
    return alg, exe


def run(mode, steps, tail):
    from ddsp_svc_amd import attention as AT
    AT.ATTN_TORCH_FASTER.clear()                       # measure the kernels everywhere, whatever the dispatcher would do
    dev = torch.device("cuda:0")
    events = mode == "throughput"
    tile = AT.tile()
    doc = {"mode": mode, "D": D, "d": DH, "m": M, "heads": HEADS, "steps": steps, "timed_over_last": tail, "tile": tile,
           "peak_tflops": PEAK_TFLOPS, "timing": "device events" if events else "host clock + synchronise",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": []}
    g = torch.Generator().manual_seed(1)
    mk = lambda *s, std: (torch.randn(*s, generator=g) * std).to(dev)
    proj = mk(M, DH, std=1.0)
    inner = HEADS * DH
    w = (mk(inner, D, std=D ** -0.5), mk(inner, std=0.1), mk(inner, D, std=D ** -0.5), mk(inner, std=0.1),
         mk(inner, D, std=D ** -0.5), mk(inner, std=0.1), mk(D, inner, std=inner ** -0.5), mk(D, std=0.1))
    with torch.no_grad():
        for B, N in SHAPES[mode]:
            gen = torch.Generator().manual_seed(B + N)
            x = torch.randn(B, N, D, generator=gen).to(dev)
            q, k, v = (torch.randn(B, HEADS, N, DH, generator=gen).to(dev) for _ in range(3))
            out = torch.empty(B, N, inner, device=dev)
            cases = (("fast_attention", lambda: AT.fast_attention(q, k, v, proj, out=out), lambda: torch_fast(q, k, v, proj)),
                     ("self_attention", lambda: AT.self_attention(x, *w, proj, heads=HEADS), lambda: torch_self(x, w, proj)))
            chunks = AT.default_chunks(B, HEADS, N)
            for name, hip, ref in cases:
                r = compare(hip, ref, steps, tail, events)
                alg, exe = flops(B, N)
                r.update(case=name, B=B, L=N, frames=B * N, launches_hip=2, key_chunks=chunks,
                         workgroups=[B * HEADS * chunks, B * HEADS * -(-N // tile)], flops_cover="the two attention kernels",
                         flops_algorithmic=alg, flops_executed=exe,
                         hip_tflops_algorithmic=alg / r["hip_ms"] * 1e-9, hip_tflops_executed=exe / r["hip_ms"] * 1e-9)
                r["fraction_of_peak_algorithmic"] = r["hip_tflops_algorithmic"] / PEAK_TFLOPS
                r["fraction_of_peak_executed"] = r["hip_tflops_executed"] / PEAK_TFLOPS
                doc["cases"].append(r)
                print(json.dumps(r), flush=True)
            del x, q, k, v, out
            AT.release_workspace()
            torch.cuda.empty_cache()
    slower = [c["frames"] for c in doc["cases"] if c["case"] == "fast_attention" and c["torch_over_hip"] < 1.0]
    doc["torch_faster_frames"] = sorted(set(slower))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("latency", "throughput", "both"), default="both")
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--tail", type=int, default=40)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_bench: needs the GPU (no fallback)")
    os.makedirs(args.out_dir, exist_ok=True)
    for mode in (("throughput", "latency") if args.mode == "both" else (args.mode,)):
        doc = run(mode, args.steps, min(args.tail, args.steps))
        path = os.path.join(args.out_dir, "attention_%s.json" % mode)
        with open(path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        print("wrote", path, flush=True)


if __name__ == "__main__":
    main()
