"""Band-limited resampling on one GPU: the HIP kernel (ddsp_svc_amd.resample) against torchaudio's op sequence (F.pad + strided
conv1d + interleave + cut, restated as resample._apply_torch) with the same float32 bank, lowpass_filter_width=128 (the
reference's setting), alternated in one process.

  --part throughput   B = 32 x 10 s: device-event time of back-to-back calls, samples/s, and the f32 MFMA-rate fraction on the
                      live-tap FLOPs (2 x outputs x live taps per phase, over 157.3 TFLOP/s)
                      The functional form (``resample.resample``: a bank built in float32, as torchaudio builds it, which has
                      no exact zeros and so runs every tap) is timed beside them
  --part latency      B = 1, the GUI callback's input (~2.35 s): host clock from the call to a synchronised result

Run each part under its own time limit; --out writes the JSON, and a text summary goes to stdout.
"""
import argparse
import json
import statistics
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ddsp_svc_amd import resample as R  # noqa: E402

PEAK_F32 = 157.3e12
LW = 128
THROUGHPUT = [(44100, 16000), (48000, 16000), (44100, 48000), (44100, 46700)]
LATENCY = [(44100, 16000), (48000, 16000), (44100, 48000)]
CALLBACK_S = 2.0 + 0.04 + 0.01 + 0.3                   # extra + crossfade + SOLA search + block


def live_taps(mod):
    k = mod.kernel[:, 0].detach().cpu()
    return float((k != 0).sum()) / k.shape[0]           # per phase, on average


def torch_chain(mod):
    o, n = int(mod.orig_freq) // mod.gcd, int(mod.new_freq) // mod.gcd
    return lambda x: R._apply_torch(x, o, n, mod.kernel, mod.width)


def events(fn, x, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn(x)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3          # us per call


def host_latency(fn, x):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def throughput(args):
    dev = torch.device("cuda:0")
    rows = []
    for a, b in THROUGHPUT:
        mod = R.Resample(a, b, lowpass_filter_width=LW).to(dev)
        x = torch.randn(32, 10 * a, device=dev)
        fns = {"hip": mod, "hip_functional": lambda v, a=a, b=b: R.resample(v, a, b, lowpass_filter_width=LW),
               "torch": torch_chain(mod)}
        with torch.no_grad():
            yh, yt = fns["hip"](x), fns["torch"](x)
            diff = float((yh - yt).pow(2).mean().sqrt() / yt.pow(2).mean().sqrt())
            for f in fns.values():
                for _ in range(args.warmup):
                    f(x)
            times = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, f in fns.items():
                    times[k].append(events(f, x, args.reps))
        T = yh.shape[-1]
        flop = 2.0 * 32 * T * live_taps(mod)
        hip_us, torch_us = statistics.median(times["hip"]), statistics.median(times["torch"])
        fun_us = statistics.median(times["hip_functional"])
        rows.append(dict(orig=a, new=b, B=32, L=10 * a, T=T, live_taps_per_phase=live_taps(mod), K=int(mod.kernel.shape[-1]),
                         hip_us=hip_us, torch_us=torch_us, hip_functional_us=fun_us, hip_us_all=times["hip"],
                         hip_functional_us_all=times["hip_functional"], torch_us_all=times["torch"],
                         speedup=torch_us / hip_us, hip_samples_per_s=32 * T / (hip_us * 1e-6),
                         live_gflop=flop / 1e9, hip_tflops=flop / (hip_us * 1e-6) / 1e12,
                         mfma_f32_fraction=flop / (hip_us * 1e-6) / PEAK_F32, rel_rms_hip_vs_torch=diff))
        print("throughput %5d -> %5d  B=32 x 10 s: HIP %9.1f us  torch %9.1f us  (x%.2f)  %.2f TFLOP/s live = %.3f of f32 MFMA peak"
              "  hip/torch rel rms %.1e;  functional form (float32 bank, every tap) %9.1f us"
              % (a, b, hip_us, torch_us, torch_us / hip_us, flop / (hip_us * 1e-6) / 1e12, flop / (hip_us * 1e-6) / PEAK_F32, diff,
                 fun_us), flush=True)
    return rows


def latency(args):
    dev = torch.device("cuda:0")
    rows = []
    for a, b in LATENCY:
        mod = R.Resample(a, b, lowpass_filter_width=LW).to(dev)
        x = torch.randn(1, int(round(CALLBACK_S * a)), device=dev)
        fns = {"hip": mod, "torch": torch_chain(mod)}
        with torch.no_grad():
            for f in fns.values():
                for _ in range(args.warmup):
                    f(x)
            times = {k: [] for k in fns}
            for _ in range(args.calls):
                for k, f in fns.items():
                    times[k].append(host_latency(f, x))
        hip_us, torch_us = statistics.median(times["hip"]), statistics.median(times["torch"])
        rows.append(dict(orig=a, new=b, B=1, L=x.shape[1], hip_us=hip_us, torch_us=torch_us,
                         hip_p90_us=sorted(times["hip"])[int(0.9 * len(times["hip"]))],
                         torch_p90_us=sorted(times["torch"])[int(0.9 * len(times["torch"]))], speedup=torch_us / hip_us))
        print("latency    %5d -> %5d  B=1 x %d: HIP %8.1f us  torch %8.1f us  (x%.2f)" % (a, b, x.shape[1], hip_us, torch_us,
                                                                                        torch_us / hip_us), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--part", choices=["throughput", "latency"], required=True)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7, help="throughput: alternated rounds")
    ap.add_argument("--reps", type=int, default=20, help="throughput: back-to-back calls per timed round")
    ap.add_argument("--calls", type=int, default=300, help="latency: timed calls per mode")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: needs the GPU (nothing measured)")
    rows = throughput(args) if args.part == "throughput" else latency(args)
    res = dict(part=args.part, device=torch.cuda.get_device_name(0), torch=torch.__version__, lowpass_filter_width=LW,
               peak_f32_tflops=PEAK_F32 / 1e12, rows=rows, args=vars(args))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
