// THE run-split rule of the overlap-add / overlap-save launchers (plain C++: no HIP, no knob(), so a host-only test can include it).
// A launcher splits an utterance's block pairs into runs, one workgroup per run, so that all workgroups are resident in ONE round
// with equal work.  A run's first tap spectrum comes out of a differently packed transform, so the LAST BITS of a filter's output
// depend on the split: two launches give the same samples only if they split alike.  That is why the rule is written once, here,
// and why a sub-batch of a split call passes the WHOLE call's batch (api.hip, lanes): its samples are then the unsplit call's bit
// for bit.  tests/test_run_split.py pins the numbers.
#pragma once

namespace ddsp {

struct RunSplit { int run, runs_per_utt; };   // most pairs a workgroup owns; workgroups per utterance = ceil(pairs / run)

// slots: workgroups resident at once; batch: utterances that share them; sharers: jobs that share the round (grid.y);
// min_run: fewest pairs worth a run's warm-up; forced_run: the launcher's *_RUN knob (< 1: none), which overrides min_run
inline RunSplit run_split(int pairs, long slots, long batch, int sharers, int min_run, long forced_run) {
  long per_utt = slots / (sharers * (batch > 0 ? batch : 1));
  if (per_utt < 1) per_utt = 1;
  int run = (int)((pairs + per_utt - 1) / per_utt);
  if (run < min_run) run = min_run;
  if (forced_run >= 1) run = (int)forced_run;
  if (run > pairs) run = pairs;
  return RunSplit{run, (pairs + run - 1) / run};
}

}  // namespace ddsp
