#!/usr/bin/env python
"""The WaveNet residual layer at C = 384 and C = 512 (H = 256) on one MI355X: the HIP path (ddsp_svc_amd.wavenet) against the
same op chain as torch ops under PyTorch-ROCm (linear / add / conv1d k = 3 / conv1d k = 1 / add / split / sigmoid / tanh / mul /
conv1d k = 1 / split / add / scale, restated here) on the same GPU in the same process with the same weights, the two alternated
step by step.

  throughput   one layer and the 20-layer stack at B x T = 64 x 862 (cfg 5), 32 x 862 and 48 x 172 (2 s training crops), device
               events around each call  -> profiles/wavenet_throughput.json
  latency      the same two at B x T = 1 x 100 (the streaming shape) and 1 x 203 (the GUI's 2.35 s window), call to result: a
               host clock around the call and a device synchronise  -> profiles/wavenet_latency.json
  split        three sides -- the torch chain, the tiled form and the channel-split form (csrc/wavenet_split.h) -- at B x T =
               1 x 100, 1 x 203, 1 x 862, 4 x 203 and 48 x 172, one layer and the 20-layer stack, alternated step by step, call
               to result; split and tiled outputs must be torch.equal in every case  -> profiles/wavenet_split_latency.json;
               ``split_below`` there is what wavenet.SPLIT_BELOW is filled from.  Not part of ``both``: it leaves the two files
               above as they are.

Each pair runs --steps alternated steps and is timed over the LAST --tail of them: the first ones run on a clock that is still
settling (EXPERIMENTS.md 6.1), so a ramp of matrix products runs first.  The achieved fraction of the 155 TF f32 MFMA peak is
reported twice: on the algorithmic flops, 2 * 2 C (4 C + H) per frame and layer, and on the flops the kernel executes (whole tiles
of 64 frames).  ``torch_faster_frames`` lists, per C, the sizes B T at which torch was faster: what LAYER_TORCH_FASTER is filled
from.  Every (mode, C) runs in a child process of its own under a time limit; a child that fails ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

H = 256
CHANNELS = (384, 512)
LAYERS = 20
PEAK_TFLOPS = 155.0                                    # measured f32 MFMA peak of one MI355X
SHAPES = {"throughput": ((64, 862), (32, 862), (48, 172)), "latency": ((1, 100), (1, 203)),
          "split": ((1, 100), (1, 203), (1, 862), (4, 203), (48, 172))}
STEP_LIMIT_S = 240                                     # per child


def make_layer(dev, C, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, std: (torch.randn(*s, generator=g) * std).to(dev)
    weights = (mk(2 * C, C, 3, std=0.75 * (3.75 * C) ** -0.5), mk(2 * C, std=0.1), mk(2 * C, H, 1, std=0.6 * H ** -0.5),
               mk(2 * C, std=0.1), mk(2 * C, C, 1, std=3.2 * C ** -0.5), mk(2 * C, std=0.1))
    return weights, (mk(C, C, std=0.5 * C ** -0.5), mk(C, std=0.1))


def torch_layer(x, cond, s, layer):
    (wdil, bdil, wc, bc, wo, bo), (wp, bp) = layer
    C = x.shape[1]
    d = F.linear(s, wp, bp).unsqueeze(-1)
    y = F.conv1d(x + d, wdil, bdil, padding=1) + F.conv1d(cond, wc, bc)
    gate, filt = torch.split(y, [C, C], dim=1)
    y = F.conv1d(torch.sigmoid(gate) * torch.tanh(filt), wo, bo)
    res, skip = torch.split(y, [C, C], dim=1)
    return (x + res) / 2.0 ** 0.5, skip


def torch_stack(x, cond, s, layers):
    skips = []
    for layer in layers:
        x, skip = torch_layer(x, cond, s, layer)
        skips.append(skip)
    return x, torch.sum(torch.stack(skips), dim=0)


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
    diff = max(float((a - b).abs().max() / b.pow(2).mean().sqrt()) for a, b in zip(yh, yt))
    del yh, yt
    th, tt = [], []
    for _ in range(steps):
        th.append(timed(hip, events))
        tt.append(timed(ref, events))
    q = lambda v: [float(np.percentile(v[-tail:], p)) * 1e3 for p in (50, 10, 90)]
    (hm, hl, hh), (tm, tl, tu) = q(th), q(tt)
    return {"hip_ms": hm, "hip_ms_p10_p90": [hl, hh], "torch_ms": tm, "torch_ms_p10_p90": [tl, tu], "torch_over_hip": tm / hm,
            "hip_ms_first_steps": float(np.median(th[:5])) * 1e3, "max_abs_diff_over_rms": diff}


def compare3(sides, steps, tail):
    """alternated: torch, tiled, split, torch, ...; call to result; the median and spread of each over the last ``tail`` steps.
    ``sides``: name -> callable returning (x_out, skip)."""
    out = {k: [t.clone() for t in fn()] for k, fn in sides.items()}
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out["split"], out["tiled"])), "the split and the tiled form differ"
    r = {"split_equals_tiled": True,
         "max_abs_diff_over_rms": max(float((a - b).abs().max() / b.pow(2).mean().sqrt()) for a, b in zip(out["split"], out["torch"]))}
    del out
    times = {k: [] for k in sides}
    for _ in range(steps):
        for k, fn in sides.items():
            times[k].append(timed(fn, False))
    for k, v in times.items():
        m, lo, hi = [float(np.percentile(v[-tail:], p)) * 1e3 for p in (50, 10, 90)]
        r[k + "_ms"], r[k + "_ms_p10_p90"] = m, [lo, hi]
    r["fastest"] = min(sides, key=lambda k: r[k + "_ms"])
    return r


def run_split(C, steps, tail):
    from ddsp_svc_amd import wavenet as WN
    dev = torch.device("cuda:0")
    layers = [make_layer(dev, C, 10 + i) for i in range(LAYERS)]
    cases = []
    ramp(dev)
    with torch.no_grad():
        for B, T in SHAPES["split"]:
            gen = torch.Generator().manual_seed(B + T)
            x, cond = torch.randn(B, C, T, generator=gen).to(dev), torch.randn(B, H, T, generator=gen).to(dev)
            s = torch.randn(B, C, generator=gen).to(dev)
            out, skip = torch.empty_like(x), torch.empty_like(x)
            w0, (wp0, bp0) = layers[0]
            layer = lambda form: lambda: WN.residual_layer(x, cond, torch.addmm(bp0, s, wp0.t()), w0, out=out, skip=skip, form=form)
            stack = lambda form: lambda: WN.residual_stack(x, cond, s, layers, form=form)
            todo = (("layer", 1, steps, {"torch": lambda: torch_layer(x, cond, s, layers[0]), "tiled": layer("tiled"),
                                         "split": layer("split")}),
                    ("stack20", LAYERS, max(steps // 4, 8), {"torch": lambda: torch_stack(x, cond, s, layers), "tiled": stack("tiled"),
                                                             "split": stack("split")}))
            for name, n, k, sides in todo:
                r = compare3(sides, k, min(tail, k))
                r.update(case=name, C=C, B=B, T=T, frames=B * T, steps=k, launches_tiled=n, launches_split=2 * n,
                         tiles_split=B * -(-T // 16), workspace_bytes_split=B * T * C * 4)
                cases.append(r)
                print(json.dumps(r), flush=True)
            del x, cond, out, skip
            WN.release_workspace()
            torch.cuda.empty_cache()
    return {"tile": WN.tile(C, H), "tile_split": WN.split_tile(C, H), "device": torch.cuda.get_device_name(0),
            "torch": torch.__version__, "cases": cases}


def split_below(cases):
    """C -> the smallest measured size at which the split form was not the fastest of the three (one past the largest measured
    size if it was the fastest at all of them); no entry if it is not the fastest at the smallest size"""
    table = {}
    for C in sorted({c["C"] for c in cases}):
        mine = sorted((c["frames"], c["fastest"]) for c in cases if c["case"] == "layer" and c["C"] == C)
        if mine and mine[0][1] == "split":
            lost = [n for n, side in mine if side != "split"]
            table[str(C)] = lost[0] if lost else mine[-1][0] + 1
    return table


def flops(C, B, T, layers, tile):
    per_frame = 2.0 * 2 * C * (4 * C + H)
    return per_frame * B * T * layers, per_frame * B * (-(-T // tile) * tile) * layers


def ramp(dev, seconds=1.5):
    """matrix products until the clock has settled"""
    a = torch.randn(4096, 4096, device=dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(8):
            a = (a @ a) * 1e-2
        torch.cuda.synchronize()


def run(mode, C, steps, tail):
    from ddsp_svc_amd import wavenet as WN
    WN.LAYER_TORCH_FASTER.clear()                      # measure the kernel everywhere, whatever the dispatcher would do
    dev = torch.device("cuda:0")
    events = mode == "throughput"
    tile = WN.tile(C, H)
    layers = [make_layer(dev, C, 10 + i) for i in range(LAYERS)]
    cases = []
    ramp(dev)
    with torch.no_grad():
        for B, T in SHAPES[mode]:
            gen = torch.Generator().manual_seed(B + T)
            x, cond = torch.randn(B, C, T, generator=gen).to(dev), torch.randn(B, H, T, generator=gen).to(dev)
            s = torch.randn(B, C, generator=gen).to(dev)
            out, skip = torch.empty_like(x), torch.empty_like(x)
            w0, (wp0, bp0) = layers[0]

            def hip_layer():
                return WN.residual_layer(x, cond, torch.addmm(bp0, s, wp0.t()), w0, out=out, skip=skip)

            todo = (("layer", 1, steps, hip_layer, lambda: torch_layer(x, cond, s, layers[0])),
                    ("stack20", LAYERS, max(steps // 4, 8), lambda: WN.residual_stack(x, cond, s, layers),
                     lambda: torch_stack(x, cond, s, layers)))
            for name, n, k, hip, ref in todo:
                r = compare(hip, ref, k, min(tail, k), events)
                alg, exe = flops(C, B, T, n, tile)
                r.update(case=name, C=C, B=B, T=T, frames=B * T, launches_hip=n, workgroups=B * -(-T // tile), steps=k,
                         flops_algorithmic=alg, flops_executed=exe,
                         hip_tflops_algorithmic=alg / r["hip_ms"] * 1e-9, hip_tflops_executed=exe / r["hip_ms"] * 1e-9,
                         floor_ms_at_peak=alg / PEAK_TFLOPS * 1e-9)
                r["fraction_of_peak_algorithmic"] = r["hip_tflops_algorithmic"] / PEAK_TFLOPS
                cases.append(r)
                print(json.dumps(r), flush=True)
            del x, cond, out, skip
            torch.cuda.empty_cache()
    return {"tile": tile, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("latency", "throughput", "both", "split"), default="both")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--tail", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", nargs=3, metavar=("MODE", "C", "PATH"), help="internal: one (mode, C) into a JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wavenet_bench: needs the GPU (no fallback)")
    if args.child:
        mode, C, path = args.child[0], int(args.child[1]), args.child[2]
        with open(path, "w") as f:
            tail = min(args.tail, args.steps)
            json.dump(run_split(C, args.steps, tail) if mode == "split" else run(mode, C, args.steps, tail), f)
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for mode in (("throughput", "latency") if args.mode == "both" else (args.mode,)):
        events = mode == "throughput"
        doc = {"mode": mode, "C": list(CHANNELS), "H": H, "layers_of_the_stack": LAYERS, "steps": args.steps,
               "timed_over_last": args.tail, "peak_tflops": PEAK_TFLOPS,
               "timing": "device events" if events else "host clock + synchronise", "cases": []}
        stem = "wavenet_split_latency" if mode == "split" else "wavenet_%s" % mode
        for C in CHANNELS:
            part = os.path.join(args.out_dir, ".%s_%d.part" % (stem, C))
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--steps", str(args.steps),
                   "--tail", str(args.tail), "--child", mode, str(C), part]
            code = subprocess.call(cmd)
            if code != 0:
                sys.exit("wavenet_bench: %s at C = %d ended with status %d; nothing more is started" % (mode, C, code))
            with open(part) as f:
                got = json.load(f)
            os.remove(part)
            doc["cases"] += got.pop("cases")
            doc.update(got)
        if mode == "split":
            doc["split_below"] = split_below(doc["cases"])
        else:
            doc["torch_faster_frames"] = {str(C): sorted({c["frames"] for c in doc["cases"] if c["C"] == C and c["case"] == "layer"
                                                          and c["torch_over_hip"] < 1.0}) for C in CHANNELS}
        path = os.path.join(args.out_dir, "%s.json" % stem)
        with open(path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        print("wrote", path, flush=True)


if __name__ == "__main__":
    main()
