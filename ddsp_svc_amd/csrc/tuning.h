// Tuning / test knobs of the launchers (run lengths, which occupancy build of a kernel is launched, ...).  Defaults are
// the measured optima; a knob is read from its DDSP_HIP_<NAME> environment variable ONCE, when the library first needs
// it, and can be changed afterwards only through ddsp_hip_set_tuning() (include/ddsp_hip.h) -- measurement tools and the
// run-split tests use that; the launch path itself never touches the environment.
#pragma once

namespace ddsp {

enum Knob {
  KNOB_BLK_WPS = 0, KNOB_BLK_RUN, KNOB_BLK_PADLDS, KNOB_FFT_RUN, KNOB_STFT_WPS, KNOB_STFT_RUN, KNOB_MEL_WPS,
  KNOB_MEL_RUN, KNOB_FIR_MAX_SLOTS, KNOB_SINS_V1, KNOB_TAPS_GEMM, KNOB_STREAM_LAYOUT, KNOB_BLK_TURNS, KNOB_CZT_ROUNDS, KNOB_CZT_TURNS,
  KNOB_SINS_NOSKIP, KNOB_SMALL_PATH, KNOB_LANE_ROWS, KNOB_LANES, KNOB_FIR_BWD_DIRECT, KNOB_BWD_WPS, KNOB_TAPS_FULL,
  KNOB_AP_BWD_SPLIT, KNOB_SINS_SEQ, KNOB_BATCH_SPLIT,
  KNOB_COUNT
};
// RETIRED (the names stay in the table so that a stale script fails loudly): BLK_WPS and BLK_PADLDS chose and probed round 3's
// two-wave hop-block filter, SINS_V1 = 2 the 16-harmonic sinusoid bank and its adjoint.  Those kernels are gone; any non-zero
// BLK_WPS / BLK_PADLDS and SINS_V1 = 2 are refused (api.hip, knob_is_inert).  SINS_V1 = 1 (the generic bank) is live.

// a step with fewer frames than this (B F) takes the streaming-shape forms: fewer, fused launches (knob SMALL_PATH = 1: never)
constexpr long kSmallRows = 4096;

long knob(Knob k);                       // current value; 0 = unset (use the built-in default)
int knob_set(const char* name, long v);  // 0 on success, -1 for an unknown name
long knob_get(const char* name);         // value, or -1 for an unknown name

// A grid holds 65 535 workgroups in y and z.  The launchers that put the utterance index there and take a larger batch
// (resblock.h, resample.h, mel_czt.hip) go through it in chunks of this many utterances, each launch starting at a base
// utterance.  Test knob BATCH_SPLIT = 1 .. 65 535: chunks of that size, so that a handful of utterances reach the second chunk;
// 0 (unset) or any other value: 65 535.
constexpr long kMaxGridYZ = 65535;
inline long batch_split() {
  const long v = knob(KNOB_BATCH_SPLIT);
  return v >= 1 && v <= kMaxGridYZ ? v : kMaxGridYZ;
}

}  // namespace ddsp
