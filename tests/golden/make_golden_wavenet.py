"""Fixture of the diffusion denoiser's WaveNet residual layer, computed by the REFERENCE itself on the CPU: ``diffusion.wavenet``'s
``ResidualBlock`` and ``WaveNet``, unmodified, with seeded weights loaded.

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the output is committed, so the tests never need it.

  wavenet_layer.npz   C = 32, H = 16 (the classes are generic, so the file stays at 150 KB), B = 2, T = 70.
                      layer_*: one ResidualBlock(16, 32, 1): x, cond, s, wdil, bdil, wc, bc, wo, bo, wp, bp -> x_out, skip.
                      net_*: WaveNet(8, 3, 32, 16): spec [2, 1, 8, 70], step [2], cond; layer i holds seeded_weights(32, 16, 10 + i) and
                      seeded_projection(32, 20 + i), which the test regenerates (they would be most of the file);
                      x0 and s are what the first residual layer received and skip_in what skip_projection received (read by
                      forward pre-hooks: the classes' code is untouched); sp_w, sp_b, op_w, op_b the two projections behind
                      the layers (output_projection's weight is seeded: the reference initialises it to zero); y the output.
                      Weights from tests/wavenet_oracle.seeded_weights: the default initialisation would leave the residual
                      at a few per cent of x.

Run:  python tests/golden/make_golden_wavenet.py
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

C, H, M, N, B, T = 32, 16, 8, 3, 2, 70
NAMES = ("wdil", "bdil", "wc", "bc", "wo", "bo")


def main():
    from tests import wavenet_oracle as O
    from tests.wavenet_standin import load
    sys.path.insert(0, REF)
    import diffusion.wavenet as W
    rng = np.random.default_rng(41)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    rec = {}
    x, cond, s = f32(B, C, T), f32(B, H, T), f32(B, C)
    weights, proj = O.seeded_weights(C, H, 1), O.seeded_projection(C, 2)
    block = load(W.ResidualBlock(H, C, 1).eval(), weights, proj)
    with torch.no_grad():
        x_out, skip = block(torch.from_numpy(x), torch.from_numpy(cond), torch.from_numpy(s))
    rec.update(layer_x=x, layer_cond=cond, layer_s=s, layer_wp=proj[0], layer_bp=proj[1], layer_x_out=x_out.numpy(),
               layer_skip=skip.numpy())
    rec.update({"layer_" + n: a for n, a in zip(NAMES, weights)})

    net = W.WaveNet(M, N, C, H).eval()
    for i, layer in enumerate(net.residual_layers):
        weights, proj = O.seeded_weights(C, H, 10 + i), O.seeded_projection(C, 20 + i)
        load(layer, weights, proj)
    with torch.no_grad():
        net.output_projection.weight.copy_(torch.from_numpy(f32(M, C, 1) * np.float32(C ** -0.5)))
    seen = {}
    net.residual_layers[0].register_forward_pre_hook(lambda mod, args: seen.update(x0=args[0], s=args[2]))
    net.skip_projection.register_forward_pre_hook(lambda mod, args: seen.update(skip_in=args[0]))
    spec, step, cond = f32(B, 1, M, T), np.array([3.0, 47.0], np.float32), f32(B, H, T)
    with torch.no_grad():
        y = net(torch.from_numpy(spec), torch.from_numpy(step), torch.from_numpy(cond))
    rec.update(net_spec=spec, net_step=step, net_cond=cond, net_x0=seen["x0"].numpy(), net_s=seen["s"].numpy(),
               net_skip_in=seen["skip_in"].numpy(), net_y=y.numpy(),
               net_sp_w=net.skip_projection.weight.detach().numpy(), net_sp_b=net.skip_projection.bias.detach().numpy(),
               net_op_w=net.output_projection.weight.detach().numpy(), net_op_b=net.output_projection.bias.detach().numpy())
    path = os.path.join(HERE, "wavenet_layer.npz")
    np.savez_compressed(path, **rec)
    print({n: v.shape for n, v in rec.items() if n.startswith(("layer_x", "layer_skip", "net_y", "net_skip"))},
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
