"""Call-to-result latency of the real-time splice: the GUI's torch chain (gui.py:431-456, phase_vocoder gui.py:15-32, restated op
for op in tests/splice_oracle.py) against ``splice.StreamingSplice``, alternated in one process on the MI355X.

A timed call starts behind a device synchronise and ends when the output block is in the callback's host ``outdata [Bf, 2]``
(the torch chain: ``.repeat(1, 2).cpu().numpy()`` as the GUI; the session: ``.cpu().numpy()`` into both channels), then a
synchronise.  The GUI's ``print`` of the shift is left out of both.  The torch chain edits its audio in place, as the GUI does,
so it gets a fresh copy of each block, made outside the timed window.  Consecutive blocks are one block apart plus a seeded
jitter within the search range, so that the searches find nonzero offsets.  Shape: B = 1, 44.1 kHz, block 0.3 s, search 0.01 s, delay
0.02 s, L = 101 888 (the model's output for the GUI's 101 430-sample input_frame at hop 512); crossfade 0.04 s without and with
the vocoder, and 0.15 s with it.

    python tools/splice_latency.py [--iters 2000] [--warmup 200] [--out profiles/splice_latency.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddsp_svc_amd import splice  # noqa: E402
from tests.splice_oracle import AtenSplice  # noqa: E402  (the GUI's op sequence, restated)

SR, L = 44100, 101888


class HipSession:
    def __init__(self, Bf, C, S, D, fade_in, fade_out, use_pv, dev):
        self.s = splice.StreamingSplice(1, Bf, C, S, D, fade_in, fade_out, use_pv, device=dev)

    def __call__(self, audio, outdata):
        out, shift = self.s(audio)
        outdata[:] = out.cpu().numpy()[:, None]
        return shift


def signal(n, seed, dev):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f0 = 160.0 + 50.0 * np.sin(2 * np.pi * 0.8 * t)
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(rng.uniform(0.1, 0.4) / h * np.sin(h * ph + rng.uniform(0, 2 * np.pi)) for h in range(1, 9))
    return torch.from_numpy((x + 0.02 * rng.standard_normal(n)).astype(np.float32)).to(dev)


def run_config(crossfade_time, use_pv, iters, warmup, dev):
    Bf, C, S, D = (int(t * SR) for t in (0.3, crossfade_time, 0.01, 0.02))
    fade_in = torch.sin(np.pi * torch.arange(0, 1, 1 / C, device=dev) / 2) ** 2    # gui.py:366-368
    fade_out = 1 - fade_in
    # the model's output of consecutive callbacks: windows of one long signal, one block apart plus a seeded jitter < search
    rng = np.random.default_rng(2)
    nb = 16
    src = signal(L + (nb + 1) * Bf, 1, dev)
    starts = [i * Bf + int(rng.integers(0, S)) for i in range(nb)]
    blocks = [src[st: st + L].contiguous() for st in starts]
    chain = AtenSplice(Bf, C, S, D, fade_in, fade_out, use_pv)
    hip = HipSession(Bf, C, S, D, fade_in, fade_out, use_pv, dev)
    out_t, out_h = np.zeros((Bf, 2), np.float32), np.zeros((Bf, 2), np.float32)
    # agreement over consecutive callbacks from the same zero tail
    check = []
    for i in range(8):
        st = chain(blocks[i].clone(), out_t)
        sh = int(hip(blocks[i], out_h))
        d = float(np.max(np.abs(out_t - out_h)))
        check.append({"shift_torch": st, "shift_hip": sh, "max_abs_diff": d, "bit_identical": bool(np.array_equal(out_t, out_h))})
    times = {"torch": [], "hip": []}
    runners = {"torch": chain, "hip": hip}
    outs = {"torch": out_t, "hip": out_h}
    for i in range(warmup + iters):
        order = ("torch", "hip") if i % 2 == 0 else ("hip", "torch")
        x = blocks[i % nb]
        for name in order:
            xin = x.clone() if name == "torch" else x          # the chain's own copy, made before the clock starts
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runners[name](xin, outs[name])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= warmup:
                times[name].append((t1 - t0) * 1e6)
    res = {"block": Bf, "crossfade": C, "search": S, "delay": D, "L": L, "use_phase_vocoder": use_pv, "iters": iters,
           "warmup": warmup, "first_calls": check}
    for name, v in times.items():
        v = np.array(v)
        res[name + "_us"] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)),
                             "p90": float(np.percentile(v, 90)), "min": float(v.min()), "max": float(v.max())}
    res["speedup_median"] = res["torch_us"]["median"] / res["hip_us"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splice_latency: needs the GPU")
    dev = torch.device("cuda:0")
    rows = [run_config(cf, pv, a.iters, a.warmup, dev) for cf, pv in ((0.04, False), (0.04, True), (0.15, True))]
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "configs": rows}
    for r in rows:
        print("crossfade %5d pv %d: torch chain %8.1f us (p10 %.1f, p90 %.1f)   StreamingSplice %7.1f us (p10 %.1f, p90 %.1f)   x%.2f"
              % (r["crossfade"], r["use_phase_vocoder"], r["torch_us"]["median"], r["torch_us"]["p10"], r["torch_us"]["p90"],
                 r["hip_us"]["median"], r["hip_us"]["p10"], r["hip_us"]["p90"], r["speedup_median"]))
        print("   first calls:", r["first_calls"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"splice_latency": [{k: r[k] for k in ("crossfade", "use_phase_vocoder", "speedup_median")} for r in rows]}))


if __name__ == "__main__":
    main()
