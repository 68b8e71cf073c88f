"""Fixture of the performer attention, computed by the REFERENCE itself on the CPU: ``ddsp.pcmer``'s ``FastAttention`` and
``SelfAttention``, unmodified.  ``gin`` and ``local_attention`` are stubbed in ``sys.modules`` (neither is reached: no local heads).

Runs only where the reference checkout is available (DDSP_REFERENCE_PATH); the output is committed, so the tests never need it.

  performer_attention.npz   small generic sizes (the classes are generic in dim_heads, so the file stays at tens of KB):
                            FastAttention(dim_heads=16) (44 features) on q, k, v [2, 3, 37, 16]: fast_proj, fast_q / _k / _v,
                            fast_y (FLAG_PCMER_NORM off) and fast_y_norm (on);
                            SelfAttention(dim=32, heads=2, dim_head=16) on self_x [2, 37, 32]: self_proj, self_w0 .. self_w7 =
                            (wq, bq, wk, bk, wv, bv, wo, bo) from tests/attention_oracle.seeded_linear, self_y.

Run:  python tests/golden/make_golden_attention.py
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

REF = os.environ.get("DDSP_REFERENCE_PATH", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from tests import attention_oracle as O
    for name in ("gin", "local_attention"):
        sys.modules.setdefault(name, MagicMock())
    sys.path.insert(0, REF)
    import ddsp.pcmer as M
    torch.manual_seed(0)
    rec = {}
    fast = M.FastAttention(dim_heads=16).eval()
    assert tuple(fast.projection_matrix.shape) == (44, 16)
    q, k, v = O.seeded_qkv(2, 3, 37, 16, seed=5)
    rec.update(fast_proj=fast.projection_matrix.numpy().copy(), fast_q=q, fast_k=k, fast_v=v)
    with torch.no_grad():
        for tag, flag in (("fast_y", False), ("fast_y_norm", True)):
            M.FLAG_PCMER_NORM = flag
            rec[tag] = fast(torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v)).numpy()
        M.FLAG_PCMER_NORM = False
        att = M.SelfAttention(dim=32, heads=2, dim_head=16).eval()
        weights = O.seeded_linear(32, 2, 16, seed=6)
        for lin, w, b in zip((att.to_q, att.to_k, att.to_v, att.to_out), weights[0::2], weights[1::2]):
            assert tuple(lin.weight.shape) == w.shape
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        x = np.random.default_rng(7).standard_normal((2, 37, 32)).astype(np.float32)
        rec.update(self_x=x, self_proj=att.fast_attention.projection_matrix.numpy().copy(), self_y=att(torch.from_numpy(x)).numpy())
        rec.update({"self_w%d" % i: a for i, a in enumerate(weights)})
    path = os.path.join(HERE, "performer_attention.npz")
    np.savez_compressed(path, **rec)
    print({n: a.shape for n, a in rec.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
