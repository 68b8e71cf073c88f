"""Latency and bandwidth of the frame-feature kernels (ddsp_svc_amd.features) against the same mathematics as torch ops on the same
GPU (tests/features_oracle.py ``aten_*``), alternated in one process on the MI355X.

B = 1, call to result, at the GUI callback's 2.35 s window (44.1 kHz, hop 512; the track from a 10 ms grid): a timed call starts
behind a device synchronise and ends behind the next one, the result on the device.  ``volume`` is also timed against the
reference's numpy loop on the host (ddsp/vocoder.py:151-157), for scale.  B = 32 x 10 s, CUDA events round ten back-to-back
launches (the host's time per call hides behind the queue): ``volume`` and ``gate`` (the C calls) with their algorithmic bytes
(4 B T and 8 B T plus the frames) as a fraction of the HBM roof, and ``signal.mul_(mask)`` on a precomputed mask (12 B T) in the
same run.

    python tools/features_latency.py [--iters 500] [--warmup 50] [--out profiles/features_latency.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddsp_svc_amd import features  # noqa: E402
from tests import features_oracle as O  # noqa: E402

SR, HOP, DB = 44100, 512, -45
HBM_ROOF_GBS = 8000.0                                    # MI355X HBM3E peak, the roof DESIGN.md uses


def numpy_volume(audio, hop):
    """Volume_Extractor.extract, restated"""
    n_frames = int(len(audio) // hop) + 1
    a2 = np.pad(audio ** 2, (hop // 2, (hop + 1) // 2), mode="reflect")
    return np.sqrt(np.array([np.mean(a2[n * hop: (n + 1) * hop]) for n in range(n_frames)]))


def stats(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)),
            "min": float(v.min())}


def wall(runners, iters, warmup, sync=True):
    """alternate the runners; each call timed from behind a synchronise to behind the next"""
    times = {k: [] for k in runners}
    names = list(runners)
    for i in range(warmup + iters):
        for name in (names if i % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runners[name]()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= warmup:
                times[name].append((t1 - t0) * 1e6)
    return {k: stats(v) for k, v in times.items()}


def events(runners, iters, warmup, inner=10):
    """CUDA events round ``inner`` back-to-back calls, so that the host's own time per call hides behind the queue"""
    times = {k: [] for k in runners}
    names = list(runners)
    for i in range(warmup + iters):
        for name in (names if i % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                runners[name]()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b) * 1e3 / inner)
    return {k: stats(v) for k, v in times.items()}


def test_signal(B, T, dev, seed=0):
    rng = np.random.default_rng(seed)
    env = np.repeat(np.where(rng.uniform(size=(B, T // 4096 + 1)) < 0.5, 0.1, 1e-4), 4096, axis=1)[:, :T]
    return torch.from_numpy((env * rng.standard_normal((B, T))).astype(np.float32)).to(dev)


def salience(N, dev, seed=1):
    rng = np.random.default_rng(seed)
    h = (rng.uniform(0, 0.02, (1, N, 360)) ** 2).astype(np.float32)
    c = (180 + 60 * np.sin(np.arange(N) / 9.0)).astype(int)
    for i in range(N):
        h[0, i] += (0.6 * np.exp(-0.5 * ((np.arange(360) - c[i]) / 1.3) ** 2)).astype(np.float32)
    h[0, N // 3: N // 3 + 12] *= 0.01                     # an unvoiced stretch
    h[0, :3] *= 0.01
    return torch.from_numpy(h).to(dev)


def run_b1(iters, warmup, dev):
    T = int(2.35 * SR) // HOP * HOP                      # the callback's window, whole hops
    F = T // HOP + 1
    N = int(T / SR / 0.01) + 1
    audio = test_signal(1, T, dev)
    hidden = salience(N, dev)
    sess = features.StreamingFeatures(1, T, HOP, N, 0.01, SR, HOP, DB, uv_interp=True, f0_min=50.0, device=dev)
    vol = sess.volume(audio[0]).clone()
    sig = torch.randn(1, F * HOP, device=dev)
    # agreement of the two sides before anything is timed
    check = {"volume_max_rel": float(((O.aten_volume(audio, HOP) - vol) / vol.clamp(min=1e-12)).abs().max()),
             "gate_max_abs": float((O.aten_gate(sig, vol[None], DB, HOP) - features.gate(sig, vol[None], DB, HOP)).abs().max()),
             "track_max_rel": float(((O.aten_track(O.aten_decode(hidden), 0.01, HOP, SR, F, True, 50.0)
                                      - sess.track(features.decode_salience(hidden)[0])[None]) / 50.0).abs().max())}
    host = audio[0].cpu().numpy()
    res = {"T": T, "frames": F, "N_src": N, "agreement": check}
    res["volume_us"] = wall({"hip": lambda: sess.volume(audio[0]), "torch": lambda: O.aten_volume(audio, HOP)}, iters, warmup)
    s_h, s_t = sig.clone(), sig.clone()
    res["gate_us"] = wall({"hip": lambda: sess.gate_(s_h[0]), "torch": lambda: s_t.mul_(O.aten_mask(vol[None], DB, HOP))},
                          iters, warmup)
    res["f0_track_us"] = wall({"hip": lambda: sess.track(features.decode_salience(hidden)[0]),
                               "torch": lambda: O.aten_track(O.aten_decode(hidden), 0.01, HOP, SR, F, True, 50.0)}, iters, warmup)
    t = []
    for _ in range(20):
        t0 = time.perf_counter()
        numpy_volume(host, HOP)
        t.append((time.perf_counter() - t0) * 1e6)
    res["volume_numpy_host_us"] = stats(t)
    for k in ("volume", "gate", "f0_track"):
        res[k + "_speedup_median"] = res[k + "_us"]["torch"]["median"] / res[k + "_us"]["hip"]["median"]
    return res


def run_batch(iters, warmup, dev):
    B, T = 32, 10 * SR // HOP * HOP
    F = T // HOP + 1
    audio = test_signal(B, T, dev, 2)
    vol = features.volume(audio, HOP)
    sig = torch.randn(B, F * HOP, device=dev)
    mask = features.silence_mask(vol, DB, HOP)
    out = torch.empty(B, F, device=dev)
    from ddsp_svc_amd import _ffi
    lib, st = _ffi.lib(), _ffi.stream_of(audio)
    t = events({"volume": lambda: lib.ddsp_hip_volume(audio.data_ptr(), T, B, T, HOP, out.data_ptr(), st),
                "gate": lambda: lib.ddsp_hip_gate(sig.data_ptr(), F * HOP, vol.data_ptr(), B, F, HOP, features.threshold_of(DB), 4,
                                                  sig.data_ptr(), F * HOP, st),
                "mul_mask": lambda: sig.mul_(mask)}, iters, warmup)
    n = B * F * HOP
    byts = {"volume": 4 * B * T + 4 * B * F, "gate": 8 * n + 4 * B * F, "mul_mask": 12 * n}
    res = {"B": B, "T": T, "frames": F, "hbm_roof_GBs": HBM_ROOF_GBS}
    for k, v in t.items():
        gbs = byts[k] / (v["median"] * 1e-6) / 1e9
        res[k] = {"us": v, "bytes": byts[k], "GBs": gbs, "roof_fraction": gbs / HBM_ROOF_GBS}
    res["gate_vs_mul_mask"] = t["mul_mask"]["median"] / t["gate"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("features_latency: needs the GPU")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "warmup": a.warmup,
              "b1": run_b1(a.iters, a.warmup, dev), "batch": run_batch(max(a.iters // 5, 20), max(a.warmup // 5, 5), dev)}
    b1, bt = result["b1"], result["batch"]
    print("B = 1, %d samples, %d frames, call to result (median us): agreement %s" % (b1["T"], b1["frames"], b1["agreement"]))
    for k in ("volume", "gate", "f0_track"):
        print("  %-9s hip %7.1f   torch ops %7.1f   x%.2f" % (k, b1[k + "_us"]["hip"]["median"], b1[k + "_us"]["torch"]["median"],
                                                                b1[k + "_speedup_median"]))
    print("  volume, the reference's numpy loop on the host: %.1f us" % b1["volume_numpy_host_us"]["median"])
    print("B = %d x %d samples (CUDA events, median):" % (bt["B"], bt["T"]))
    for k in ("volume", "gate", "mul_mask"):
        print("  %-9s %8.1f us  %7.1f GB/s  %.3f of the %.0f GB/s roof" % (k, bt[k]["us"]["median"], bt[k]["GBs"],
                                                                        bt[k]["roof_fraction"], HBM_ROOF_GBS))
    print("  gate against signal.mul_(mask): x%.2f" % bt["gate_vs_mul_mask"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"features_latency": {k: b1[k + "_speedup_median"] for k in ("volume", "gate", "f0_track")},
                      "gate_vs_mul_mask": bt["gate_vs_mul_mask"]}))


if __name__ == "__main__":
    main()
