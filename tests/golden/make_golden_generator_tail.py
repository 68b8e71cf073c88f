"""Fixture of the NSF-HiFiGAN generator's upsampling seams and output head, computed by the REFERENCE itself on the CPU:
``nsf_hifigan.models.Generator``, unmodified, with weight norm removed, seeded weights and a seeded stand-in for the harmonic
source (the reference's draws noise on every call).

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the output is committed, so the tests never need it.

  generator_tail.npz   num_mels 8, 64 initial channels, upsample rates [2, 2], kernels [4, 4], B = 2, 20 frames.  Forward hooks
                       record, per seam i, the input of ``ups[i]`` (``up_in_<i>``: already through lrelu 0.1), and the input of
                       the stage's first residual block (``stage_in_<i>``: the seam's output); the output of ``conv_pre``
                       (``pre_out``, whose lrelu is ``up_in_0``); the source (``source``); the input of ``conv_post``
                       (``post_in``: already through lrelu 0.01) and the generator's output (``out``).  With them the weights
                       of ``ups``, ``noise_convs`` and ``conv_post`` (``wu_<i>``, ``bu_<i>``, ``wn_<i>``, ``bn_<i>``, ``wp``, ``bp``).
                       Those weights are the oracle's seeded ones at std 1 / sqrt(fan-in) with biases at std 0.1: the
                       reference's own init of ``ups`` and ``conv_post`` (std 0.01) would leave every convolution's sum far
                       below its bias and the fixture blind to a wrong tap or weight order.  The residual blocks keep their
                       init (close to the identity), so the activations stay of order one up to the head.

Run:  python tests/golden/make_golden_generator_tail.py
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

B, FRAMES = 2, 20


def import_reference():
    sys.path.insert(0, REF)
    for m in ["matplotlib", "matplotlib.pylab"]:
        sys.modules.setdefault(m, MagicMock())
    import nsf_hifigan.models as models
    from nsf_hifigan.env import AttrDict
    return models, AttrDict


class Source(torch.nn.Module):
    def forward(self, f0, upp):
        g = torch.Generator().manual_seed(5)
        return torch.randn(f0.shape[0], f0.shape[1] * upp, 1, generator=g).to(f0)


def main():
    from tests import generator_tail_oracle as O
    models, AttrDict = import_reference()
    h = AttrDict(num_mels=8, upsample_initial_channel=64, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], resblock="1",
                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, sampling_rate=44100)
    torch.manual_seed(3)
    gen = models.Generator(h).eval()
    gen.remove_weight_norm()
    gen.m_source = Source()
    rec = {}
    with torch.no_grad():
        for i, (Cout, s) in enumerate(((32, 2), (16, 1))):
            wu, bu, wn, bn = O.seeded_seam_weights(Cout, 2, s, seed=30 + i)
            for t, a in ((gen.ups[i].weight, wu), (gen.ups[i].bias, bu), (gen.noise_convs[i].weight, wn), (gen.noise_convs[i].bias, bn)):
                assert tuple(t.shape) == a.shape, (t.shape, a.shape)
                t.copy_(torch.from_numpy(a))
            rec.update({"wu_%d" % i: wu, "bu_%d" % i: bu, "wn_%d" % i: wn, "bn_%d" % i: bn})
        wp, bp = O.seeded_head_weights(16, seed=40)
        gen.conv_post.weight.copy_(torch.from_numpy(wp))
        gen.conv_post.bias.copy_(torch.from_numpy(bp))
        rec.update(wp=wp, bp=bp)

        def keep(name, what):
            def hook(module, args, output=None):
                rec[name] = (output if what == "out" else args[0]).detach().numpy().copy()
            return hook
        gen.conv_pre.register_forward_hook(keep("pre_out", "out"))
        gen.conv_post.register_forward_pre_hook(keep("post_in", "in"))
        gen.noise_convs[0].register_forward_pre_hook(keep("source", "in"))
        for i in range(2):
            gen.ups[i].register_forward_pre_hook(keep("up_in_%d" % i, "in"))
            gen.resblocks[3 * i].register_forward_pre_hook(keep("stage_in_%d" % i, "in"))
        g = torch.Generator().manual_seed(4)
        mel, f0 = 2.0 * torch.randn(B, 8, FRAMES, generator=g), torch.full((B, FRAMES), 220.0)
        rec["out"] = gen(mel, f0).numpy()
    path = os.path.join(HERE, "generator_tail.npz")
    np.savez_compressed(path, **rec)
    print({n: v.shape for n, v in rec.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
