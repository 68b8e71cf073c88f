"""Fixture of the NSF-HiFiGAN residual block, computed by the REFERENCE itself on the CPU: ``nsf_hifigan.models.ResBlock1``,
unmodified, with weight norm removed and seeded weights.

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the output is committed, so the tests never need it.

  resblock1.npz   C = 16, k in {3, 7, 11}, dilations (1, 3, 5), x [2, 16, 150]: x, and per k the twelve weight / bias arrays
                  (w1_<k>_<pair>, b1_..., w2_..., b2_...) and the block's output y_<k>.  Weights at std 1 / sqrt(C k), biases at
                  std 0.1: the reference's own init (std 0.01) would make every term but the residual vanish.

Run:  python tests/golden/make_golden_resblock.py
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

C, T, B, DIL = 16, 150, 2, (1, 3, 5)


def import_reference():
    sys.path.insert(0, REF)
    for m in ["matplotlib", "matplotlib.pylab"]:
        sys.modules.setdefault(m, MagicMock())
    import nsf_hifigan.models as models
    return models


def main():
    from tests import resblock_oracle as O
    models = import_reference()
    rng = np.random.default_rng(20)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    rec = {"x": x}
    for k in (3, 7, 11):
        blk = models.ResBlock1(None, C, k, DIL)
        blk.remove_weight_norm()
        weights = O.seeded_weights(C, k, len(DIL), seed=100 + k)
        with torch.no_grad():
            for p, (w1, b1, w2, b2) in enumerate(weights):
                blk.convs1[p].weight.copy_(torch.from_numpy(w1))
                blk.convs1[p].bias.copy_(torch.from_numpy(b1))
                blk.convs2[p].weight.copy_(torch.from_numpy(w2))
                blk.convs2[p].bias.copy_(torch.from_numpy(b2))
                rec.update({"w1_%d_%d" % (k, p): w1, "b1_%d_%d" % (k, p): b1, "w2_%d_%d" % (k, p): w2, "b2_%d_%d" % (k, p): b2})
            rec["y_%d" % k] = blk(torch.from_numpy(x)).numpy()
    path = os.path.join(HERE, "resblock1.npz")
    np.savez_compressed(path, **rec)
    print({n: v.shape for n, v in rec.items() if n[0] in "xy"}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
