#!/usr/bin/env python
"""The conformer conv module at D = 256 on one MI355X: the HIP path (ddsp_svc_amd.conformer) against the same op chain as torch
ops under PyTorch-ROCm (layer_norm / transpose / conv1d / glu / grouped conv1d / silu / conv1d / transpose / add, restated here)
on the same GPU in the same process with the same weights, the two alternated step by step.

  throughput   one module and the 3-layer conv-only encoder at B = 32 x 862 frames (10 s) and B = 48 x 172 (2 s training crops),
               device events around each call  -> profiles/conformer_throughput.json
  latency      the same two at B = 1 x 100 (the streaming shape) and B = 1 x 203 frames (the GUI's 2.35 s window), call to
               result: a host clock around the call and a device synchronise  -> profiles/conformer_latency.json
  split        three sides -- the torch chain, the tiled form and the channel-split form (csrc/conformer_split.h) -- at B x L =
               1 x 100, 1 x 203, 4 x 203, 1 x 862 and 48 x 172, the module, the module with LayerNorm and the 3-layer encoder,
               alternated step by step, call to result  -> profiles/conformer_split_latency.json; ``split_below`` there is what
               conformer.CONV_SPLIT_BELOW is filled from.  Not part of ``both``: it leaves the two files above as they are.

Each pair runs --steps alternated steps and is timed over the LAST --tail of them: the first hundred or so run on a clock that is
still settling (EXPERIMENTS.md 6.1); the split mode runs a ramp of matrix products first.  The achieved fraction of the 155 TF f32 MFMA peak is reported twice: on the algorithmic
flops, 2 (D 4 D + 2 D 31 + 2 D D) per frame and layer, and on the flops the kernel executes (GEMM 1 on 128 frames and GEMM 2 on
112 per tile of 98).  ``crossover`` lists, per D, the largest B L at which torch was faster: what CONV_TORCH_FASTER is filled from.
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

D = 256
TAPS = 31
PEAK_TFLOPS = 155.0                                    # measured f32 MFMA peak of one MI355X
SHAPES = {"throughput": ((32, 862), (48, 172)), "latency": ((1, 100), (1, 203)),
          "split": ((1, 100), (1, 203), (4, 203), (1, 862), (48, 172))}


def make_layer(dev, seed, use_norm):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, std: (torch.randn(*s, generator=g) * std).to(dev)
    I = 2 * D
    weights = (mk(2 * I, D, 1, std=1.6 * D ** -0.5), mk(2 * I, std=0.1), mk(I, 1, TAPS, std=1.8 * TAPS ** -0.5), mk(I, std=0.1),
               mk(D, I, 1, std=I ** -0.5), mk(D, std=0.1))
    norm = (1.0 + mk(D, std=0.3), mk(D, std=0.2)) if use_norm else None
    return weights, norm, 1e-5


def torch_net(x, layer):
    (w1, b1, wd, bd, w2, b2), norm, eps = layer
    h = x if norm is None else F.layer_norm(x, (D,), norm[0], norm[1], eps)
    h = F.glu(F.conv1d(h.transpose(1, 2), w1, b1), dim=1)
    h = F.silu(F.conv1d(h, wd, bd, padding=TAPS // 2, groups=2 * D))
    return F.conv1d(h, w2, b2).transpose(1, 2)


def torch_encoder(x, layers):
    for layer in layers:
        x = x + torch_net(x, layer)
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


def compare3(sides, steps, tail):
    """alternated: torch, tiled, split, torch, ...; call to result; the median and spread of each over the last ``tail`` steps.
    ``sides``: name -> callable returning [B, L, D]."""
    out = {k: fn().clone() for k, fn in sides.items()}
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


def split_below(cases):
    """D -> the smallest measured size at which the split form was not the fastest of the three for the plain module (one past
    the largest measured size if it was the fastest at all of them); no entry if it is not the fastest at the smallest size"""
    mine = sorted((c["frames"], c["fastest"]) for c in cases if c["case"] == "module")
    if not mine or mine[0][1] != "split":
        return {}
    lost = [n for n, side in mine if side != "split"]
    return {str(D): lost[0] if lost else mine[-1][0] + 1}


def ramp(dev, seconds=1.5):
    """matrix products until the clock has settled"""
    a = torch.randn(4096, 4096, device=dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(8):
            a = (a @ a) * 1e-2
        torch.cuda.synchronize()


def run_split(steps, tail):
    from ddsp_svc_amd import conformer as CF
    dev = torch.device("cuda:0")
    doc = {"mode": "split", "D": D, "steps": steps, "timed_over_last": tail, "tile": CF.tile(D), "tile_split": CF.split_tile(D),
           "timing": "host clock + synchronise", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": []}
    layers = [make_layer(dev, 10 + i, False) for i in range(3)]
    normed = make_layer(dev, 20, True)
    ramp(dev)
    with torch.no_grad():
        for B, L in SHAPES["split"]:
            x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(B + L)).to(dev)
            out = torch.empty_like(x)
            module = lambda form: lambda: CF.conv_module(x, layers[0][0], out=out, form=form)
            module_norm = lambda form: lambda: CF.conv_module(x, normed[0], norm=normed[1], out=out, form=form)
            enc = lambda form: lambda: CF.encoder(x, layers, out=out, form=form)
            todo = (("module", 1, steps, lambda: torch_net(x, layers[0]), module),
                    ("module_norm", 1, steps, lambda: torch_net(x, normed), module_norm),
                    ("encoder3", 3, max(steps // 2, 8), lambda: torch_encoder(x, layers), enc))
            for name, n, k, ref, hip in todo:
                r = compare3({"torch": ref, "tiled": hip("tiled"), "split": hip("split")}, k, min(tail, k))
                r.update(case=name, D=D, B=B, L=L, frames=B * L, steps=k, launches_tiled=n, launches_split=3 * n,
                         tiles_split=B * -(-L // 16), workspace_bytes_split=4 * B * L * D * 4)
                doc["cases"].append(r)
                print(json.dumps(r), flush=True)
            del x, out
            CF.release_workspace()
            torch.cuda.empty_cache()
    doc["split_below"] = split_below(doc["cases"])
    return doc


def flops(B, L, layers, tile):
    per_frame = 2.0 * (D * 4 * D + 2 * D * TAPS + 2 * D * D)
    tiles = -(-L // tile)
    executed = 2.0 * (D * 4 * D * 128 + 2 * D * TAPS * tile + 2 * D * D * 112) * tiles
    return per_frame * B * L * layers, executed * B * layers


def run(mode, steps, tail):
    from ddsp_svc_amd import conformer as CF
    CF.CONV_TORCH_FASTER.clear()                       # measure the kernel everywhere, whatever the dispatcher would do
    dev = torch.device("cuda:0")
    events = mode == "throughput"
    tile = CF.tile(D)
    doc = {"mode": mode, "D": D, "steps": steps, "timed_over_last": tail, "tile": tile, "peak_tflops": PEAK_TFLOPS,
           "timing": "device events" if events else "host clock + synchronise", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "cases": []}
    layers = [make_layer(dev, 10 + i, False) for i in range(3)]      # Unit2Control(use_naive_v2=True): conv only, no norm
    normed = make_layer(dev, 20, True)                                # the conv half of a PCmer layer
    with torch.no_grad():
        for B, L in SHAPES[mode]:
            x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(B + L)).to(dev)
            out = torch.empty_like(x)
            cases = (("module", 1, lambda: CF.conv_module(x, layers[0][0], out=out), lambda: torch_net(x, layers[0])),
                     ("module_norm", 1, lambda: CF.conv_module(x, normed[0], norm=normed[1], out=out), lambda: torch_net(x, normed)),
                     ("encoder3", 3, lambda: CF.encoder(x, layers, out=out), lambda: torch_encoder(x, layers)))
            for name, n, hip, ref in cases:
                r = compare(hip, ref, steps, tail, events)
                alg, exe = flops(B, L, n, tile)
                r.update(case=name, B=B, L=L, frames=B * L, launches_hip=n, workgroups=B * -(-L // tile),
                         flops_algorithmic=alg, flops_executed=exe,
                         hip_tflops_algorithmic=alg / r["hip_ms"] * 1e-9, hip_tflops_executed=exe / r["hip_ms"] * 1e-9)
                r["fraction_of_peak_algorithmic"] = r["hip_tflops_algorithmic"] / PEAK_TFLOPS
                r["fraction_of_peak_executed"] = r["hip_tflops_executed"] / PEAK_TFLOPS
                doc["cases"].append(r)
                print(json.dumps(r), flush=True)
            del x, out
            torch.cuda.empty_cache()
    slower = [c["frames"] for c in doc["cases"] if c["case"].startswith("module") and c["torch_over_hip"] < 1.0]
    doc["torch_faster_frames"] = sorted(set(slower))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("latency", "throughput", "both", "split"), default="both")
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--tail", type=int, default=40)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conformer_bench: needs the GPU (no fallback)")
    os.makedirs(args.out_dir, exist_ok=True)
    for mode in (("throughput", "latency") if args.mode == "both" else (args.mode,)):
        tail = min(args.tail, args.steps)
        doc = run_split(args.steps, tail) if mode == "split" else run(mode, args.steps, tail)
        path = os.path.join(args.out_dir, "conformer_split_latency.json" if mode == "split" else "conformer_%s.json" % mode)
        with open(path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        print("wrote", path, flush=True)


if __name__ == "__main__":
    main()
