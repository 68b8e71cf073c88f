"""Fixtures of the real-time splice, computed by the REFERENCE itself: ``GUI.audio_callback`` (gui.py:393-456) and
``phase_vocoder`` (gui.py:15-32) of the unmodified reference module, on the CPU.

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the outputs are committed, so the tests never need it.
The GUI's third-party imports are stubbed in ``sys.modules``; ``self`` is a stand-in whose ``svc_model.infer`` returns seeded audio:
consecutive windows of one seeded signal, each advanced by a block plus a small seeded jitter, so that SOLA has an offset to find.

  splice_plain.npz   four callbacks, crossfade without the phase vocoder
  splice_pv.npz      four callbacks with the phase vocoder
  splice_short.npz   four callbacks with block < crossfade (the output is all crossfade, the new tail partly), plain
  splice_pv_direct.npz   phase_vocoder alone at an even and an odd length

Each callback records the model's audio, the output block (outdata[:, 0]), the tail after the call and the shift printed by the
callback.  Run:  python tests/golden/make_golden_splice.py
"""
import contextlib
import io
import os
import re
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    # name: (block, crossfade, search, delay, use_phase_vocoder, seed)
    "splice_plain": (256, 128, 48, 32, False, 11),
    "splice_pv": (256, 128, 48, 32, True, 12),
    "splice_short": (64, 160, 40, 24, False, 13),
}
CALLS = 4


def import_gui():
    sys.path.insert(0, REF)
    for m in ["FreeSimpleGUI", "sounddevice", "librosa", "enhancer", "torchaudio", "torchaudio.transforms",
              "ddsp", "ddsp.vocoder", "ddsp.core"]:
        sys.modules.setdefault(m, MagicMock())
    sys.modules["librosa"].to_mono = lambda y: np.mean(y, axis=0) if y.ndim > 1 else y
    import gui
    return gui


def seeded_signal(n, seed):
    """a few drifting partials plus noise: periodic enough that the SOLA search has a real optimum"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    f0 = 180.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 2 * np.pi))
    ph = 2 * np.pi * np.cumsum(f0) / 44100.0
    x = sum(rng.uniform(0.1, 0.5) / h * np.sin(h * ph + rng.uniform(0, 2 * np.pi)) for h in range(1, 7))
    return (x + 0.02 * rng.standard_normal(n)).astype(np.float32)


def run_case(gui, Bf, C, S, D, use_pv, seed):
    L = Bf + C + S + D + 3 * Bf
    rng = np.random.default_rng(seed + 1000)
    sig = seeded_signal(L + (CALLS + 1) * Bf + 64, seed)
    starts = [c * Bf + int(rng.integers(0, 32)) for c in range(CALLS)]
    audios = [sig[s: s + L].copy() for s in starts]
    calls = iter(audios)

    me = types.SimpleNamespace()
    me.block_frame, me.crossfade_frame, me.sola_search_frame, me.last_delay_frame = Bf, C, S, D
    me.input_wav = np.zeros(L, dtype=np.float32)
    me.config = types.SimpleNamespace(samplerate=44100, spk_id=1, threhold=-60, f_pitch_change=0, use_spk_mix=False,
                                      spk_mix_dict=None, use_vocoder_based_enhancer=False, select_pitch_extractor="rmvpe",
                                      use_phase_vocoder=use_pv)
    me.f_safe_prefix_pad_length = 0.0
    me.resample_kernel = {}
    me.device = "cpu"
    me.svc_model = types.SimpleNamespace(infer=lambda *a, **k: (torch.from_numpy(next(calls).copy()), 44100))
    me.sola_buffer = torch.zeros(C)
    me.fade_in_window = torch.sin(np.pi * torch.arange(0, 1, 1 / C) / 2) ** 2      # gui.py:366-368
    me.fade_out_window = 1 - me.fade_in_window
    rec = {"audio": np.stack(audios), "fade_in": me.fade_in_window.numpy(), "fade_out": me.fade_out_window.numpy(),
           "sizes": np.array([Bf, C, S, D, int(use_pv)], np.int64)}
    outs, bufs, shifts = [], [], []
    for _ in range(CALLS):
        outdata = np.zeros((Bf, 2), np.float32)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            gui.GUI.audio_callback(me, np.zeros((Bf, 1), np.float32), outdata, Bf, None, None)
        shifts.append(int(re.search(r"sola_shift: (-?\d+)", log.getvalue()).group(1)))
        outs.append(outdata[:, 0].copy())
        bufs.append(me.sola_buffer.numpy().copy())
    rec.update(out=np.stack(outs), buffer=np.stack(bufs), shift=np.array(shifts, np.int64))
    return rec


def main():
    gui = import_gui()
    torch.manual_seed(0)
    for name, (Bf, C, S, D, use_pv, seed) in CASES.items():
        rec = run_case(gui, Bf, C, S, D, use_pv, seed)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(name, "shifts", rec["shift"].tolist(), os.path.getsize(path), "bytes")
    rng = np.random.default_rng(21)
    direct = {}
    for n in (96, 77):
        fi = torch.sin(np.pi * torch.arange(0, 1, 1 / n) / 2) ** 2
        a = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        direct.update({"a%d" % n: a.numpy(), "b%d" % n: b.numpy(), "fade_in%d" % n: fi.numpy(), "fade_out%d" % n: (1 - fi).numpy(),
                       "out%d" % n: gui.phase_vocoder(a, b, 1 - fi, fi).numpy()})
    path = os.path.join(HERE, "splice_pv_direct.npz")
    np.savez_compressed(path, **direct)
    print("splice_pv_direct", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
