"""Write tests/golden/phase_parent_noinfer.npz: phase0 (float64), x and a CombSub signal (float32) of the training path
(``infer=False``) at F = 1 and 17, hop 512, B = 2 with an initial phase, as ``compute_noinfer`` of tests/test_phase_sum_first.py forms
them on an MI355X.  The arrays in the repository were recorded from the build of commit 435e383, the parent of the change that moved
the ``infer`` path to "sum first, scale once": the training path must stay at these bits.  Run it at the commit whose numbers are to be
kept, or against that commit's library through ``DDSP_HIP_LIB``:

    python tests/golden/make_golden_phase_noinfer.py [output.npz]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.test_phase_sum_first import NOINFER_FILE, compute_noinfer  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the recorded bits are an MI355X's"
    out = compute_noinfer(torch.device("cuda:0"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", NOINFER_FILE)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: (v.dtype.name, v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
