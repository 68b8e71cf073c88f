"""The tap syntheses of csrc/ir_pfa.hip (k_taps_pfa510 and the fused front launch k_front_small) against arrays RECORDED from the
build of commit b29e10c on an MI355X (tests/golden/front_parent_taps.npz): index and idle-wave work of the kernel may be
rearranged, its numbers may not move -- every tap and the CombSub signal behind them are compared as uint32 views, bit for bit.

Kinds: all-pass / roll, real (exp activation) / Hann in full rows -- and in half rows and full rows through the fused front path --,
real / dynamic window with half widths on both sides of N/2 = 255 and one row below 0.5 (its batch takes the per-tap window form).
Row counts 1, 15, 16, 17, 33: the batch edges of the 16-row workgroup (a batch of one row, a partial one, full ones), where the
number of threads and waves that hold an item of the two DFT stages changes."""
import numpy as np
import pytest
import torch

SR, HOP, NB, NT = 44100, 512, 256, 510
ROW_COUNTS = (1, 15, 16, 17, 33)
FUSED_F = 17
GOLDEN_FILE = "front_parent_taps.npz"


def _controls(rows, seed):
    return np.random.default_rng(seed).standard_normal((rows, NB)).astype(np.float32)


def _half_widths(rows, seed):
    hw = (np.random.default_rng(seed).random(rows) * 520 + 60).astype(np.float32)      # 60 .. 580: both sides of 255
    if rows >= 16:
        hw[rows - 1] = np.float32(0.3)                                              # < 0.5: the last batch takes the per-tap form
    return hw


def _operator_taps(dev):
    """the three kinds through the per-operator entry points (k_taps_pfa510), every row count"""
    from ddsp_svc_amd import _ffi, core
    lib = _ffi.lib()
    tab = core.ir_table(NB, dev)
    out = {}
    for rows in ROW_COUNTS:
        ctrl = torch.from_numpy(_controls(rows, 1000 + rows)).to(dev)
        hw = torch.from_numpy(_half_widths(rows, 2000 + rows)).to(dev)
        st = _ffi.stream_of(ctrl)
        taps = torch.empty(rows, NT, dtype=torch.float32, device=dev)
        nbytes = lib.ddsp_hip_allpass_taps_scratch_bytes(rows, NB)
        scratch = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        _ffi.check(lib.ddsp_hip_allpass_taps(ctrl.data_ptr(), NB, rows, NB, tab.data_ptr(), taps.data_ptr(), scratch.data_ptr(),
                                             nbytes, st))
        out["allpass_%d" % rows] = taps.cpu().numpy().copy()
        _ffi.check(lib.ddsp_hip_impulse_response(ctrl.data_ptr(), NB, None, 0, _ffi.ACT_EXP, 1.0 / 128, _ffi.MODE_HANN, None, rows,
                                                 NB, tab.data_ptr(), taps.data_ptr(), st))
        out["hann_%d" % rows] = taps.cpu().numpy().copy()
        _ffi.check(lib.ddsp_hip_impulse_response(ctrl.data_ptr(), NB, None, 0, _ffi.ACT_EXP, 1.0, _ffi.MODE_DYNAMIC, hw.data_ptr(),
                                                 rows, NB, tab.data_ptr(), taps.data_ptr(), st))
        out["dynamic_%d" % rows] = taps.cpu().numpy().copy()
    return out


def _fused_front(dev, set_knob):
    """a small CombSub call (one utterance of 17 frames: a full batch and a batch of one row): exciter and the three tap syntheses in
    k_front_small; the taps are read where the call leaves them in its workspace (ddsp_hip_tail_layout)"""
    from ddsp_svc_amd import synth
    F = FUSED_F
    rng = np.random.default_rng(77)
    f0 = np.exp(rng.uniform(np.log(100.0), np.log(800.0), (1, F))).astype(np.float32)    # half widths 66150 / f0: 83 .. 660
    cg, ch, cn = (rng.standard_normal((1, F, NB)).astype(np.float32) for _ in range(3))
    u = rng.random((1, F * HOP), dtype=np.float32)
    f0t, cgt, cht, cnt, ut = (torch.from_numpy(a).to(dev) for a in (f0, cg, ch, cn, u))
    out = {}
    for full in (0, 1):
        set_knob("TAPS_FULL", full)
        sess = synth.StreamingCombSub(1, F, NB, NB, NB, SR, HOP, dev, want_components=True)
        sess._ws.zero_()
        sess.phase(f0t)
        sig, _, _ = sess.synth(f0t, cgt, cht, cnt, ut, noise_is_u01=True)
        lay = synth._tail_layout(True, 1, F, HOP, NB, NB, NB)
        assert lay is not None and min(lay[2], lay[3], lay[4]) >= 0
        tag = "full" if full else "half"
        out["fused_%s_signal" % tag] = sig.cpu().numpy().copy()
        out["fused_%s_allpass" % tag] = synth._ws_view(sess._ws, lay[2], (F, NT)).cpu().numpy().copy()
        out["fused_%s_dynamic" % tag] = synth._ws_view(sess._ws, lay[3], (F, NT)).cpu().numpy().copy()
        out["fused_%s_noise" % tag] = synth._ws_view(sess._ws, lay[4], (F, NT if full else NB)).cpu().numpy().copy()
    return out


def compute(dev, set_knob):
    out = _operator_taps(dev)
    out.update(_fused_front(dev, set_knob))
    return out


# the fused call's results are the same arrays in both layouts (asserted below), so the file holds them once
STORED_ONCE = {"fused_full_signal": "fused_half_signal", "fused_full_allpass": "fused_half_allpass",
               "fused_full_dynamic": "fused_half_dynamic"}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def recorded(golden_dir):
    import os
    with np.load(os.path.join(golden_dir, GOLDEN_FILE)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def computed():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddsp_svc_amd import _ffi
    touched = []

    def set_knob(name, value):
        assert _ffi.lib().ddsp_hip_set_tuning(name.encode(), int(value)) == 0, name
        touched.append(name)
    try:
        return compute(torch.device("cuda:0"), set_knob)
    finally:
        for name in touched:
            _ffi.lib().ddsp_hip_set_tuning(name.encode(), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["allpass", "hann", "dynamic"])
def test_operator_taps_are_the_recorded_bits(computed, recorded, kind):
    for rows in ROW_COUNTS:
        key = "%s_%d" % (kind, rows)
        assert np.isfinite(computed[key]).all(), key
        assert same_bits(computed[key], recorded[key]), key


@pytest.mark.gpu
def test_fused_front_taps_and_signal_are_the_recorded_bits(computed, recorded):
    for key in [k for k in computed if k.startswith("fused_")]:
        assert same_bits(computed[key], recorded[STORED_ONCE.get(key, key)]), key
    # the fused launch is the per-operator kernel with an exciter job beside it: the half rows are the full rows' first N/2 + 1 taps
    assert same_bits(computed["fused_half_noise"], computed["fused_full_noise"][:, :NB])
    assert float(np.abs(computed["fused_half_signal"]).sum()) > 0


@pytest.mark.gpu
def test_real_response_full_rows_exactly_even(computed):
    """row k1 = 0 of the DFT-30 stage holds tap j and tap N - j of its own, equal to rounding only: the one at j <= N/2 serves
    both, so a zero-phase response under the (even) Hann window is even bit for bit"""
    j = np.arange(1, NT)
    for key in ["hann_%d" % r for r in ROW_COUNTS] + ["fused_full_noise"]:
        t = computed[key]
        assert same_bits(t[:, j], t[:, NT - j]), key
