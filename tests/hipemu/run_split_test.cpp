// ddsp_svc_amd/csrc/run_split.h behind a C symbol, for tests/test_run_split.py.  TEST INFRASTRUCTURE ONLY.
#include "run_split.h"

extern "C" void emu_run_split(int pairs, long slots, long batch, int sharers, int min_run, long forced_run, int* out) {
  const ddsp::RunSplit r = ddsp::run_split(pairs, slots, batch, sharers, min_run, forced_run);
  out[0] = r.run;
  out[1] = r.runs_per_utt;
}
