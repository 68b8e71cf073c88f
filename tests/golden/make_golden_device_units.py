"""Write tests/golden/device_units.npz: what the plain C++ twins of the packed complex helpers (ddsp_svc_amd/csrc/fft2048.h, the
bodies the CPU emulator compiles) give on the seeded records of tests/device_units/helper_cases.py.  tests/test_device_units.py
holds the emulator AND the MI355X to these bits.

    python tests/golden/make_golden_device_units.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.device_units import helper_cases as hc  # noqa: E402
from tests.device_units.backend import load  # noqa: E402


def main():
    units = load("emu")
    out = {}
    for name in hc.HELPERS:
        rec = hc.random_records(name)
        out["rand_" + name] = hc.pack(name, rec, hc.run(units, name, rec))
        out["spec_" + name] = hc.run(units, name, hc.special_records(name))
    path = os.path.join(ROOT, "tests", "golden", "device_units.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
