#!/usr/bin/env python
"""The layer of the reflow / diffusion-fast denoiser at (D, Hc) = (512, 128) on one MI355X: the HIP path (ddsp_svc_amd.naive_v2)
against the same op chain as torch ops under PyTorch-ROCm (conv1d k = 1 on the step / conv1d k = 1 on the condition / adds /
conv1d k = 1 / glu / depthwise conv1d k = 31 / silu / conv1d k = 1 / add, restated here in the reference's [B, D, L]) on the same
GPU in the same process with the same weights, the two alternated step by step.

  throughput   one layer and the 6-layer stack at B x L = 64 x 862, 32 x 862 and 48 x 172 (2 s training crops), device events
               around each call  -> profiles/naive_v2_throughput.json
  latency      the same two at B x L = 1 x 100 (the streaming shape) and 1 x 203 (the GUI's 2.35 s window), call to result: a
               host clock around the call and a device synchronise  -> profiles/naive_v2_latency.json
  split        three sides -- the torch chain, the tiled form and the channel-split form (csrc/naive_v2_split.h) -- at B x L =
               1 x 100, 1 x 203, 1 x 862, 4 x 203 and 48 x 172, one layer and the 6-layer stack, alternated step by step, call
               to result  -> profiles/naive_v2_split_latency.json; ``split_below`` there is what naive_v2.SPLIT_BELOW is
               filled from.  Not part of ``both``: it leaves the two files above as they are.

Each pair runs --steps alternated steps and is timed over the LAST --tail of them: the first ones run on a clock that is still
settling (EXPERIMENTS.md 6.1), so a ramp of matrix products runs first.  The achieved fraction of the 155 TF f32 MFMA peak is
reported twice: on the algorithmic flops, 2 (D Hc + 4 D D + 31 * 2 D + 2 D D) per frame and layer, and on the flops the kernels
execute (whole tiles of 64 frames in the first launch, of 112 in the second).  ``torch_faster_frames`` lists the sizes B L at
which torch was faster: what LAYER_TORCH_FASTER is filled from.  Every mode runs in a child process of its own under a time
limit; a child that fails ends the run.
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

D, HC = 512, 128
LAYERS = 6
PEAK_TFLOPS = 155.0                                    # measured f32 MFMA peak of one MI355X
SHAPES = {"throughput": ((64, 862), (32, 862), (48, 172)), "latency": ((1, 100), (1, 203)),
          "split": ((1, 100), (1, 203), (1, 862), (4, 203), (48, 172))}
STEP_LIMIT_S = 300                                     # per child


def make_layer(dev, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, std: (torch.randn(*s, generator=g) * std).to(dev)
    weights = (mk(D, HC, 1, std=0.6 * HC ** -0.5), mk(D, std=0.1), mk(4 * D, D, 1, std=(1.62 * D) ** -0.5), mk(4 * D, std=0.1),
               mk(2 * D, 1, 31, std=(31 * 0.293) ** -0.5), mk(2 * D, std=0.1), mk(D, 2 * D, 1, std=1.67 * (2 * D) ** -0.5),
               mk(D, std=0.1))
    return weights, (mk(D, D, 1, std=0.5 * D ** -0.5), mk(D, std=0.1))


def torch_layer(x, cond, step, layer):
    """x [B, D, L], cond [B, Hc, L], step [B, D, 1]"""
    (wc, bc, w1, b1, wd, bd, w2, b2), (wp, bp) = layer
    h = x + F.conv1d(step, wp, bp) + F.conv1d(cond, wc, bc)
    h = F.glu(F.conv1d(h, w1, b1), dim=1)
    h = F.silu(F.conv1d(h, wd, bd, padding=15, groups=2 * D))
    return x + F.conv1d(h, w2, b2)


def torch_stack(x, cond, step, layers):
    for layer in layers:
        x = torch_layer(x, cond, step, layer)
    return x


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
    """alternated: hip, torch, hip, torch, ...; the median and spread of each over the last ``tail`` steps.  ``hip`` returns
    [B, L, D], ``ref`` [B, D, L]."""
    yh, yt = hip(), ref().transpose(1, 2)
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
            "hip_ms_first_steps": float(np.median(th[:5])) * 1e3, "max_abs_diff_over_rms": diff}


def compare3(sides, steps, tail):
    """alternated: torch, tiled, split, torch, ...; call to result; the median and spread of each over the last ``tail`` steps.
    ``sides``: name -> callable returning [B, L, D]."""
    out = {k: fn() for k, fn in sides.items()}
    torch.cuda.synchronize()
    r = {"split_equals_tiled": bool(torch.equal(out["split"], out["tiled"])),
         "max_abs_diff_over_rms": float((out["split"] - out["torch"]).abs().max() / out["torch"].pow(2).mean().sqrt())}
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


def run_split(steps, tail):
    from ddsp_svc_amd import naive_v2 as NV
    dev = torch.device("cuda:0")
    layers = [make_layer(dev, 10 + i) for i in range(LAYERS)]
    cases = []
    ramp(dev)
    with torch.no_grad():
        for B, L in SHAPES["split"]:
            gen = torch.Generator().manual_seed(B + L)
            x, cond = torch.randn(B, L, D, generator=gen).to(dev), torch.randn(B, L, HC, generator=gen).to(dev)
            s = torch.randn(B, D, generator=gen).to(dev)
            xt, ct, st = x.transpose(1, 2).contiguous(), cond.transpose(1, 2).contiguous(), s.unsqueeze(-1)
            out = torch.empty_like(x)
            w0, (wp0, bp0) = layers[0]
            layer = lambda form: lambda: NV.diff_layer(x, cond, torch.addmm(bp0, s, wp0[:, :, 0].t()), w0, out=out, form=form)
            stack = lambda form: lambda: NV.diff_stack(x, cond, s, layers, form=form)
            todo = (("layer", 1, steps, {"torch": lambda: torch_layer(xt, ct, st, layers[0]).transpose(1, 2),
                                         "tiled": layer("tiled"), "split": layer("split")}),
                    ("stack6", LAYERS, max(steps // 4, 8), {"torch": lambda: torch_stack(xt, ct, st, layers).transpose(1, 2),
                                                            "tiled": stack("tiled"), "split": stack("split")}))
            for name, n, k, sides in todo:
                r = compare3(sides, k, min(tail, k))
                r.update(case=name, D=D, B=B, L=L, frames=B * L, steps=k, launches_tiled=2 * n, launches_split=4 * n,
                         tiles_split=B * -(-L // 16), workspace_bytes_split=5 * B * L * D * 4)
                cases.append(r)
                print(json.dumps(r), flush=True)
            del x, cond, xt, ct, out
            NV.release_workspace()
            torch.cuda.empty_cache()
    return {"tile": list(NV.tile(D, HC)), "tile_split": NV.split_tile(D, HC), "device": torch.cuda.get_device_name(0),
            "torch": torch.__version__, "cases": cases}


def split_below(cases):
    """D -> the smallest measured size at which the split form was not the fastest of the three (one past the largest measured
    size if it was the fastest at all of them); no entry if it is not the fastest at the smallest size"""
    table = {}
    for d in sorted({c["D"] for c in cases}):
        mine = sorted((c["frames"], c["fastest"]) for c in cases if c["case"] == "layer" and c["D"] == d)
        if mine and mine[0][1] == "split":
            lost = [n for n, side in mine if side != "split"]
            table[str(d)] = lost[0] if lost else mine[-1][0] + 1
    return table


def flops(B, L, layers, tiles):
    up = lambda t: -(-L // t) * t
    front, taps, back = 2.0 * (D * HC + 4 * D * D), 2.0 * 31 * 2 * D, 2.0 * 2 * D * D
    return (front + taps + back) * B * L * layers, (front * up(tiles[0]) + (taps + back) * up(tiles[1])) * B * layers


def ramp(dev, seconds=1.5):
    """matrix products until the clock has settled"""
    a = torch.randn(4096, 4096, device=dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(8):
            a = (a @ a) * 1e-2
        torch.cuda.synchronize()


def run(mode, steps, tail):
    from ddsp_svc_amd import naive_v2 as NV
    NV.LAYER_TORCH_FASTER.clear()                      # measure the kernels everywhere, whatever the dispatcher would do
    dev = torch.device("cuda:0")
    events = mode == "throughput"
    tiles = NV.tile(D, HC)
    layers = [make_layer(dev, 10 + i) for i in range(LAYERS)]
    cases = []
    ramp(dev)
    with torch.no_grad():
        for B, L in SHAPES[mode]:
            gen = torch.Generator().manual_seed(B + L)
            x, cond = torch.randn(B, L, D, generator=gen).to(dev), torch.randn(B, L, HC, generator=gen).to(dev)
            s = torch.randn(B, D, generator=gen).to(dev)
            xt, ct, st = x.transpose(1, 2).contiguous(), cond.transpose(1, 2).contiguous(), s.unsqueeze(-1)
            out = torch.empty_like(x)
            w0, (wp0, bp0) = layers[0]

            def hip_layer():
                return NV.diff_layer(x, cond, torch.addmm(bp0, s, wp0[:, :, 0].t()), w0, out=out)

            todo = (("layer", 1, steps, hip_layer, lambda: torch_layer(xt, ct, st, layers[0])),
                    ("stack6", LAYERS, max(steps // 4, 8), lambda: NV.diff_stack(x, cond, s, layers),
                     lambda: torch_stack(xt, ct, st, layers)))
            for name, n, k, hip, ref in todo:
                r = compare(hip, ref, k, min(tail, k), events)
                alg, exe = flops(B, L, n, tiles)
                r.update(case=name, D=D, B=B, L=L, frames=B * L, launches_hip=2 * n,
                         workgroups=[B * -(-L // tiles[0]), B * -(-L // tiles[1])], steps=k,
                         flops_algorithmic=alg, flops_executed=exe, workspace_bytes=B * L * 2 * D * 4,
                         hip_tflops_algorithmic=alg / r["hip_ms"] * 1e-9, hip_tflops_executed=exe / r["hip_ms"] * 1e-9,
                         floor_ms_at_peak=alg / PEAK_TFLOPS * 1e-9)
                r["fraction_of_peak_algorithmic"] = r["hip_tflops_algorithmic"] / PEAK_TFLOPS
                r["fraction_of_peak_executed"] = r["hip_tflops_executed"] / PEAK_TFLOPS
                cases.append(r)
                print(json.dumps(r), flush=True)
            del x, cond, xt, ct, out
            NV.release_workspace()
            torch.cuda.empty_cache()
    return {"tile": list(tiles), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("latency", "throughput", "both", "split"), default="both")
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--tail", type=int, default=40)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", nargs=2, metavar=("MODE", "PATH"), help="internal: one mode into a JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("naive_v2_bench: needs the GPU (no fallback)")
    if args.child:
        mode, path = args.child
        with open(path, "w") as f:
            tail = min(args.tail, args.steps)
            json.dump(run_split(args.steps, tail) if mode == "split" else run(mode, args.steps, tail), f)
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for mode in (("throughput", "latency") if args.mode == "both" else (args.mode,)):
        events = mode == "throughput"
        doc = {"mode": mode, "D": D, "Hc": HC, "layers_of_the_stack": LAYERS, "steps": args.steps,
               "timed_over_last": args.tail, "peak_tflops": PEAK_TFLOPS,
               "timing": "device events" if events else "host clock + synchronise", "cases": []}
        stem = "naive_v2_split_latency" if mode == "split" else "naive_v2_%s" % mode
        part = os.path.join(args.out_dir, ".%s.part" % stem)
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--steps", str(args.steps),
               "--tail", str(args.tail), "--child", mode, part]
        code = subprocess.call(cmd)
        if code != 0:
            sys.exit("naive_v2_bench: %s ended with status %d; nothing more is started" % (mode, code))
        with open(part) as f:
            got = json.load(f)
        os.remove(part)
        doc["cases"] += got.pop("cases")
        doc.update(got)
        if mode == "split":
            doc["split_below"] = split_below(doc["cases"])
        else:
            doc["torch_faster_frames"] = sorted({c["frames"] for c in doc["cases"] if c["case"] == "layer" and c["torch_over_hip"] < 1.0})
        path = os.path.join(args.out_dir, "%s.json" % stem)
        with open(path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        print("wrote", path, flush=True)


if __name__ == "__main__":
    main()
