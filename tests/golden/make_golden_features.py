"""Fixtures of the frame features, computed by the REFERENCE itself on the CPU: ``Volume_Extractor.extract`` and
``F0_Extractor.extract`` (ddsp/vocoder.py), ``SvcDDSP.infer`` (gui.py:75-147), ``to_local_average_f0`` (encoder/rmvpe/utils.py)
and the pools of ddsp/core.py, all unmodified.

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the outputs are committed, so the tests never need it.
Third-party imports are stubbed in ``sys.modules``; the networks are stand-ins that return seeded arrays:

  features_volume.npz   Volume_Extractor.extract at hops 160 and 512, T a multiple of the hop and not
  features_infer.npz    the whole of SvcDDSP.infer with a model that returns ones (so the output IS the upsampled mask), a stand-in
                        units encoder and rmvpe, use_enhancer=False, a safe prefix: the audio, the stand-in's f0, and the f0 and
                        volume handed to the model
  features_decode.npz   to_local_average_f0 on seeded salience with clipped windows, a tie, a silent row and a given center
  features_track.npz    F0_Extractor.extract: the rmvpe branch with and without uv_interp and with silence_front > 0, and the crepe
                        branch behind a stand-in torchcrepe (the real pools, threshold and index retime)
  features_pools.npz    MaskedAvgPool1d / MedianPool1d at k = 3, 4, 9 on rows with NaNs

Run:  python tests/golden/make_golden_features.py
"""
import contextlib
import io
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
SR = 44100


def import_reference():
    sys.path.insert(0, REF)
    for m in ["FreeSimpleGUI", "sounddevice", "librosa", "librosa.filters", "enhancer", "torchaudio", "torchaudio.transforms",
              "pyworld", "parselmouth", "torchcrepe", "resampy", "transformers", "fairseq", "encoder.hubert",
              "encoder.hubert.model", "ddsp.unit2control", "gui_locale", "yaml"]:
        sys.modules.setdefault(m, MagicMock())
    import ddsp.core as core
    import ddsp.vocoder as vocoder
    import encoder.rmvpe.utils as rutils
    import gui
    return core, vocoder, rutils, gui


def source_f0(n, seed, lead=3, tail=4):
    """a seeded 10 ms track: voiced stretches of a drifting pitch between unvoiced ones, unvoiced at both ends"""
    rng = np.random.default_rng(seed)
    f0 = (180.0 + 60.0 * np.sin(np.arange(n) / 7.0 + rng.uniform(0, 6)) + rng.uniform(-3, 3, n)).astype(np.float32)
    f0[:lead] = 0
    f0[n - tail:] = 0
    for _ in range(max(1, n // 16)):
        s = int(rng.integers(lead + 1, n - tail - 1))
        f0[s: s + int(rng.integers(1, 6))] = 0
    return f0


def extractor(vocoder, kind, hop, f0_min=65.0, f0_max=800.0, **attrs):
    ex = object.__new__(vocoder.F0_Extractor)
    ex.f0_extractor, ex.sample_rate, ex.hop_size, ex.f0_min, ex.f0_max = kind, SR, hop, f0_min, f0_max
    for k, v in attrs.items():
        setattr(ex, k, v)
    return ex


def golden_volume(vocoder):
    rng = np.random.default_rng(1)
    rec = {}
    for hop, T in ((160, 160 * 20), (512, 512 * 7 + 133)):
        env = np.repeat(rng.uniform(0.0, 1.0, T // 100 + 1), 100)[:T] ** 3
        audio = (env * rng.standard_normal(T)).astype(np.float32)
        audio[3 * hop: 5 * hop] = 0                          # silent frames
        rec["audio_%d" % hop] = audio
        rec["volume_%d" % hop] = vocoder.Volume_Extractor(hop).extract(audio)
    return rec


def golden_infer(vocoder, gui):
    block, frames = 256, 40
    T = block * frames + 77
    rng = np.random.default_rng(2)
    env = np.full(T, 1e-4)
    for a, b in ((700, 1100), (7400, 8300)):                 # two loud stretches; the rest lies 35 dB under the threshold
        env[a:b] = 0.1
    audio = (env * rng.standard_normal(T)).astype(np.float32)
    prefix = 0.08                                            # silence_front = 0.05 s -> start_frame 8
    start = int((prefix - 0.03) * SR / block)
    f0_src = source_f0(int((T - start * block) / SR / 0.01) + 1, 3)
    vocoder.F0_KERNEL["rmvpe"] = types.SimpleNamespace(infer_from_audio=lambda *a, **k: f0_src.copy())
    seen = {}

    def model(units, f0, volume, spk_id=None, spk_mix_dict=None):
        seen["f0"], seen["volume"] = f0[0, :, 0].numpy().copy(), volume[0, :, 0].numpy().copy()
        return torch.ones(1, f0.shape[1] * block), None, (None, None)
    me = types.SimpleNamespace(
        args=types.SimpleNamespace(data=types.SimpleNamespace(block_size=block, sampling_rate=SR)), device="cpu", model=model,
        units_encoder=types.SimpleNamespace(encode=lambda a, sr, hop: torch.zeros(1, frames + 1, 4)))
    with contextlib.redirect_stdout(io.StringIO()):
        out, sr = gui.SvcDDSP.infer(me, audio, SR, threhold=-45, pitch_extractor_type="rmvpe", f0_min=50, f0_max=1100,
                                    use_enhancer=False, safe_prefix_pad_length=prefix)
    assert sr == SR
    return {"audio": audio, "f0_src": f0_src, "mask": out.numpy(), "f0": seen["f0"], "volume": seen["volume"],
            "sizes": np.array([block, SR, -45, start, 50], np.int64)}


def golden_decode(rutils):
    rng = np.random.default_rng(4)
    N = 24
    h = (rng.uniform(0, 0.02, (1, N, 360)) ** 2).astype(np.float32)
    peaks = [0, 3, 356, 359] + [int(v) for v in rng.integers(10, 350, N - 4)]
    for i, c in enumerate(peaks):
        w = np.exp(-0.5 * ((np.arange(360) - c - rng.uniform(-0.4, 0.4)) / 1.3) ** 2)
        h[0, i] += (rng.uniform(0.2, 0.9) * w).astype(np.float32)
    h[0, 10] = 0                                             # a silent row
    h[0, 11] *= np.float32(0.01)                             # under the threshold
    h[0, 12, 200] = h[0, 12, 100] = h[0, 12].max() + np.float32(0.125)   # a tie: the first bin wins
    center = rng.integers(0, 360, (1, N, 1))
    center[0, :2, 0] = (1, 358)
    t = torch.from_numpy(h)
    return {"hidden": h, "f0": rutils.to_local_average_f0(t, thred=0.03).astype(np.float32),
            "center": center[..., 0], "f0_center": rutils.to_local_average_f0(t, center=torch.from_numpy(center), thred=0.03)
            .astype(np.float32)}


def golden_track(core, vocoder):
    rec = {}
    hop, T = 512, 512 * 60 + 200                             # 61 frames; the source below ends before the last of them
    audio = np.zeros(T, np.float32)
    silence_front = 0.06
    start = int(silence_front * SR / hop)
    f0_src = source_f0(62, 5)
    rmvpe = types.SimpleNamespace(infer_from_audio=lambda *a, **k: f0_src.copy())
    rec["rmvpe_src"] = f0_src
    rec["rmvpe_sizes"] = np.array([hop, SR, T // hop + 1, start], np.int64)
    for uv in (False, True):
        rec["rmvpe_uv%d" % uv] = extractor(vocoder, "rmvpe", hop, rmvpe=rmvpe).extract(audio, uv_interp=uv, silence_front=0)
        rec["rmvpe_front_uv%d" % uv] = extractor(vocoder, "rmvpe", hop, rmvpe=rmvpe).extract(audio, uv_interp=uv,
                                                                                           silence_front=silence_front)
    # the crepe branch: seeded f0 / periodicity on the 5 ms grid from the stand-in torchcrepe, everything behind it the reference's
    rng = np.random.default_rng(6)
    n = 130
    raw = (220.0 + 40.0 * np.sin(np.arange(n) / 9.0) + rng.uniform(-2, 2, n)).astype(np.float32)[None]
    pd = rng.uniform(0.2, 1.0, n).astype(np.float32)[None]
    for a, b in ((0, 6), (40, 52), (90, 93)):
        pd[0, a:b] = rng.uniform(0.0, 0.04, b - a)

    class At:                                                # torchcrepe.threshold.At
        def __init__(self, value):
            self.value = value

        def __call__(self, pitch, periodicity):
            pitch = torch.clone(pitch)
            pitch[periodicity < self.value] = float("nan")
            return pitch
    tc = sys.modules["torchcrepe"]
    tc.predict = lambda *a, **k: (torch.from_numpy(raw.copy()), torch.from_numpy(pd.copy()))
    tc.threshold = types.SimpleNamespace(At=At)
    kernel = types.SimpleNamespace(to=lambda dev: (lambda x: x))
    pooled = core.MaskedAvgPool1d(At(0.05)(torch.from_numpy(raw), core.MedianPool1d(torch.from_numpy(pd), 4)), 4)
    rec.update(crepe_raw=raw, crepe_pd=pd, crepe_pooled=pooled.numpy())
    for uv in (False, True):
        rec["crepe_front_uv%d" % uv] = extractor(vocoder, "crepe", hop, resample_kernel=kernel).extract(
            audio, uv_interp=uv, device="cpu", silence_front=silence_front)
    return rec


def golden_pools(core):
    rng = np.random.default_rng(7)
    x = rng.uniform(50, 400, (2, 50)).astype(np.float32)
    x[0, [0, 1, 7, 20, 21, 22, 23, 24, 49]] = np.nan
    x[1, 10:22] = np.nan                                     # windows that hold nothing but NaN
    rec = {"x": x}
    for k in (3, 4, 9):
        rec["avg_%d" % k] = core.MaskedAvgPool1d(torch.from_numpy(x), k).numpy()
        rec["median_%d" % k] = core.MedianPool1d(torch.from_numpy(x), k).numpy()
    return rec


def main():
    core, vocoder, rutils, gui = import_reference()
    torch.manual_seed(0)
    for name, rec in (("features_volume", golden_volume(vocoder)), ("features_infer", golden_infer(vocoder, gui)),
                      ("features_decode", golden_decode(rutils)), ("features_track", golden_track(core, vocoder)),
                      ("features_pools", golden_pools(core))):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(name, {k: (v.shape, str(v.dtype)) for k, v in rec.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
