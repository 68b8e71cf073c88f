"""Fixture of the reflow / diffusion-fast denoiser's layer, computed by the REFERENCE itself on the CPU: ``reflow.naive_v2_diff``'s
``NaiveV2DiffLayer`` and ``NaiveV2Diff``, unmodified, with seeded weights loaded.

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH, or a ``reference`` directory beside the repository);
the output is committed, so the tests never need it.  Needs torch and numpy only: the package itself is not imported.

  naive_v2_layer.npz  dim = 32, condition_dim = 8, mel_channels = 8 (the classes are generic, so the file stays small), B = 2,
                      L = 70, tensors in the reference's [B, channels, L].
                      layer_*: one NaiveV2DiffLayer(32, 8): x, cond, step [B, 32, 1], the eight weights, wp, bp -> y.
                      net_*: NaiveV2Diff(8, 32, use_mlp=False, condition_dim=8, num_layers=3): spec [2, 1, 8, 70], step [2], cond;
                      layer i holds seeded_weights(32, 8, 10 + i) and seeded_projection(32, 20 + i), which the test regenerates;
                      x0 and s are what the first layer received and out_in what output_projection received (read by forward
                      pre-hooks: the classes' code is untouched); op_w, op_b the output projection (its weight is seeded: the
                      reference initialises it to zero); y the output.
                      Weights from tests/naive_v2_oracle.seeded_weights: the default initialisation would leave the branch at a
                      few per cent of x.

Run:  python tests/golden/make_golden_naive_v2.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DDSP_REFERENCE_PATH", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)

D, HC, M, N, B, L = 32, 8, 8, 3, 2, 70
NAMES = ("wc", "bc", "w1", "b1", "wd", "bd", "w2", "b2")


def main():
    from tests import naive_v2_oracle as O
    sys.path.insert(0, REF)
    import reflow.naive_v2_diff as V
    rng = np.random.default_rng(43)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    rec = {}
    x, cond, step = f32(B, D, L), f32(B, HC, L), f32(B, D, 1)
    weights, proj = O.seeded_weights(D, HC, 1), O.seeded_projection(D, 2)
    layer = O.load(V.NaiveV2DiffLayer(D, HC, use_mlp=False).eval(), weights, proj)
    with torch.no_grad():
        y = layer(torch.from_numpy(x), torch.from_numpy(cond), torch.from_numpy(step))
    rec.update(layer_x=x, layer_cond=cond, layer_step=step, layer_wp=proj[0], layer_bp=proj[1], layer_y=y.numpy())
    rec.update({"layer_" + n: a for n, a in zip(NAMES, weights)})

    net = V.NaiveV2Diff(mel_channels=M, dim=D, use_mlp=False, condition_dim=HC, num_layers=N).eval()
    for i, lay in enumerate(net.residual_layers):
        O.load(lay, O.seeded_weights(D, HC, 10 + i), O.seeded_projection(D, 20 + i))
    with torch.no_grad():
        net.output_projection.weight.copy_(torch.from_numpy(f32(M, D, 1) * np.float32(D ** -0.5)))
    seen = {}
    net.residual_layers[0].register_forward_pre_hook(lambda mod, args: seen.update(x0=args[0], s=args[2]))
    net.output_projection.register_forward_pre_hook(lambda mod, args: seen.update(out_in=args[0]))
    spec, step, cond = f32(B, 1, M, L), np.array([3.0, 47.0], np.float32), f32(B, HC, L)
    with torch.no_grad():
        y = net(torch.from_numpy(spec), torch.from_numpy(step), torch.from_numpy(cond))
    rec.update(net_spec=spec, net_step=step, net_cond=cond, net_x0=seen["x0"].numpy(), net_s=seen["s"].numpy(),
               net_out_in=seen["out_in"].numpy(), net_y=y.numpy(),
               net_op_w=net.output_projection.weight.detach().numpy(), net_op_b=net.output_projection.bias.detach().numpy())
    path = os.path.join(HERE, "naive_v2_layer.npz")
    np.savez_compressed(path, **rec)
    print({n: v.shape for n, v in rec.items() if n.startswith(("layer_x", "layer_y", "net_y", "net_out"))},
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
