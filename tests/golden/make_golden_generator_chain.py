"""Fixtures of the whole NSF-HiFiGAN generator chain, computed by the REFERENCE itself on the CPU: ``nsf_hifigan.models.Generator``,
unmodified, with weight norm removed, the seeded weights of tests/generator_standin.py copied in and a stored tensor as the
harmonic source (the reference's draws noise on every call).

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the output is committed, so the tests never need it.

  generator_chain_a.npz   the stock vocoder's tail: 256 initial channels, rates [2, 2, 2, 2], B = 2, 24 frames
  generator_chain_b.npz   128 initial channels, rates [8, 4], B = 2, 20 frames

Each holds ``mel``, ``f0``, ``source`` and ``out`` of both utterances and ``stage_<i>``, the output of stage i (the input of the
next ``ups``, before its lrelu; of ``conv_post`` for the last) of UTTERANCE 0 ONLY: both utterances' boundaries would not fit the
200 000 bytes a fixture is held to.  The reference never holds a stage's output in a module's input or output -- the next
module sees it through a leaky relu, which cannot be undone to the bit -- so forward hooks copy the three blocks' outputs as they
are returned and the script repeats the reference's own float32 lines on them, ``xs = r0; xs += r1; xs += r2; xs / 3``.

All weights are the stand-in's seeded ones, at std 1 / sqrt(fan-in): the reference's init (std 0.01) would leave the blocks at the
identity and every convolution below its bias.

Run:  python tests/golden/make_golden_generator_chain.py
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

B = 2


def import_reference():
    sys.path.insert(0, REF)
    for m in ["matplotlib", "matplotlib.pylab"]:
        sys.modules.setdefault(m, MagicMock())
    import nsf_hifigan.models as models
    from nsf_hifigan.env import AttrDict
    return models, AttrDict


def main():
    from tests import generator_standin as S
    models, AttrDict = import_reference()
    for name, topo in S.TOPOLOGIES.items():
        rates = list(topo["rates"])
        h = AttrDict(num_mels=S.MELS, upsample_initial_channel=topo["C0"], upsample_rates=rates,
                     upsample_kernel_sizes=[2 * u for u in rates], resblock="1", resblock_kernel_sizes=list(S.KERNELS),
                     resblock_dilation_sizes=[list(S.DILATIONS)] * len(S.KERNELS), sampling_rate=44100)
        gen = models.Generator(h).eval()
        gen.remove_weight_norm()
        S.load_weights(gen, S.weights(name))
        mel, f0, source = S.seeded_inputs(name, B, topo["frames"])
        gen.m_source = S.StoredSource()
        gen.m_source.value = torch.from_numpy(source)
        blocks = {}
        for j, blk in enumerate(gen.resblocks):
            blk.register_forward_hook(lambda m, a, out, j=j: blocks.__setitem__(j, out.detach().clone()))
        rec = dict(mel=mel, f0=f0, source=source)
        with torch.no_grad():
            rec["out"] = gen(torch.from_numpy(mel), torch.from_numpy(f0)).numpy()
            n = gen.num_kernels
            for i in range(len(rates)):
                xs = blocks[i * n].clone()
                for j in range(1, n):
                    xs += blocks[i * n + j]
                rec["stage_%d" % i] = (xs / n)[0].numpy().copy()
        path = os.path.join(HERE, "generator_chain_%s.npz" % name)
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        print(name, {k: v.shape for k, v in rec.items()}, size, "bytes")
        assert size < 200000, size


if __name__ == "__main__":
    main()
