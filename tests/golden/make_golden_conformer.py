"""Fixture of the conformer conv module, computed by the REFERENCE itself on the CPU: ``reflow.model_conformer_naive``'s
``ConformerConvModule`` and ``ConformerNaiveEncoder``, unmodified, with seeded weights loaded.

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the output is committed, so the tests never need it.

  conformer_conv.npz   dim = 32 (the class is generic in dim, so the file stays at tens of KB), x [2, 70, 32].
                       plain_* / norm_*: one module without and with the LayerNorm: w1, b1, wd, bd, w2, b2 (+ gamma, beta) and y.
                       enc<i>_*: the weights of the three layers of ConformerNaiveEncoder(3, 8, 32, conv_only=True), enc_y its output.
                       Weights from tests/conformer_oracle.seeded_weights: the default initialisation would leave net(x) at
                       0.06 of x.

Run:  python tests/golden/make_golden_conformer.py
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

D, L, B = 32, 70, 2
NAMES = ("w1", "b1", "wd", "bd", "w2", "b2")


def _load(module, weights, norm):
    net = module.net
    with torch.no_grad():
        for p, a in zip((net[2].weight, net[2].bias, net[4].weight, net[4].bias, net[6].weight, net[6].bias), weights):
            assert tuple(p.shape) == a.shape
            p.copy_(torch.from_numpy(a))
        if norm is not None:
            net[0].weight.copy_(torch.from_numpy(norm[0]))
            net[0].bias.copy_(torch.from_numpy(norm[1]))


def main():
    from tests import conformer_oracle as O
    sys.path.insert(0, REF)
    import reflow.model_conformer_naive as M
    rng = np.random.default_rng(31)
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    rec = {"x": x}
    for tag, use_norm, seed in (("plain", False, 1), ("norm", True, 2)):
        weights = O.seeded_weights(D, seed)
        norm = O.seeded_norm(D, seed + 10) if use_norm else None
        mod = M.ConformerConvModule(D, use_norm=use_norm).eval()
        _load(mod, weights, norm)
        with torch.no_grad():
            rec[tag + "_y"] = mod(torch.from_numpy(x)).numpy()
        rec.update({"%s_%s" % (tag, n): a for n, a in zip(NAMES, weights)})
        if norm is not None:
            rec.update({tag + "_gamma": norm[0], tag + "_beta": norm[1]})
    enc = M.ConformerNaiveEncoder(3, 8, D, False, True, 0, 0.1).eval()
    for i, layer in enumerate(enc.encoder_layers):
        weights = O.seeded_weights(D, 20 + i)
        _load(layer.conformer, weights, None)
        rec.update({"enc%d_%s" % (i, n): a for n, a in zip(NAMES, weights)})
    with torch.no_grad():
        rec["enc_y"] = enc(torch.from_numpy(x)).numpy()
    path = os.path.join(HERE, "conformer_conv.npz")
    np.savez_compressed(path, **rec)
    print({n: v.shape for n, v in rec.items() if n.endswith("y") or n == "x"}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
