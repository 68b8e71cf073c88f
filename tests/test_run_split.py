"""The run-split rule of the overlap-add launchers (ddsp_svc_amd/csrc/run_split.h) against a table of recorded numbers.

A run's first tap spectrum comes out of a differently packed transform, so the last bits of a filter's output follow the split:
the bit-for-bit tests (test_small_shapes, test_lanes, test_batch_split) compare launches with each other and hold whenever the
launches agree; this one pins WHAT the rule computes.  tests/golden/run_split_table.json holds, per row,
[site, pairs, slots, batch, sharers, min_run, forced_run, run, runs_per_utt]: the arguments as each launcher derives them, and
the result of that launcher's own hand-written block as it stood before the blocks became one helper (recorded from those
blocks, not from the helper; a row that two launchers share is listed once: fir_fft's are fir_fft_bwd's, mel's are mel_bwd's).  The rows take every clamp both ways: batch above the slots (per_utt floored at 1; 65 535),
pairs 1 .. 3 under min_run 3, 4 and 6, forced_run 0, 1, 3, above pairs and negative, one and two sharers over odd and even
quotients, both sides of B F = 4096 (which switches min_run and the sharers), and B = 32, F = 862 (431 / 432 pairs).
Host code only: no kernel runs."""
import ctypes
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SITES = {"fir_blk", "fir_blk_bwd_2wave", "fir_blk_bwd_3wave", "fir_fft", "mel", "stft_filter", "stft_filter_bwd"}


@pytest.fixture(scope="module")
def run_split():
    from tests.hipemu import build as emu
    os.makedirs(emu.OUT, exist_ok=True)
    out = os.path.join(emu.OUT, "librun_split_test.so")
    deps = [os.path.join(HERE, "hipemu", "run_split_test.cpp"), os.path.join(emu.CSRC, "run_split.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run([emu._clang(), "-std=c++17", "-O2", "-fPIC", "-shared", "-I", emu.CSRC, deps[0], "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_run_split.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                ctypes.POINTER(ctypes.c_int)]
    L.emu_run_split.restype = None

    def call(pairs, slots, batch, sharers, min_run, forced_run):
        got = (ctypes.c_int * 2)()
        L.emu_run_split(pairs, slots, batch, sharers, min_run, forced_run, got)
        return got[0], got[1]
    return call


def test_run_split_table(run_split):
    with open(os.path.join(HERE, "golden", "run_split_table.json")) as f:
        table = json.load(f)
    assert len(table) >= 300 and {r[0] for r in table} == SITES
    wrong = [(r[:7], tuple(r[7:]), run_split(*r[1:7])) for r in table if run_split(*r[1:7]) != tuple(r[7:])]
    assert not wrong, "%d of %d rows differ; first (row, recorded, got): %r" % (len(wrong), len(table), wrong[0])


def test_run_split_invariants(run_split):
    """what every row of the table has in common: 1 <= run <= pairs, and the runs cover the pairs with none to spare"""
    for pairs in (1, 2, 3, 7, 431, 432):
        for batch in (1, 5, 32, 1537, 65535):
            for forced in (0, 1, 3, 1000):
                run, runs = run_split(pairs, 1536, batch, 1, 3, forced)
                assert 1 <= run <= pairs and (runs - 1) * run < pairs <= runs * run
