"""The schedule of one EM run (csrc/em_schedule.h: em_schedule) from a stand-alone C++ program that includes that header alone and
is built with AddressSanitizer and UBSan: every combination of kinds, split / unsplit, per-run state, wide rounds, second wave
stream and run counter against a restatement written here as one row of rules per kind, then the schedules that matter written
out by hand (they are what sbgpu_em_run_device* issued before the schedule was a function).  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "em_schedule.h"
#include <cstdio>
#include <vector>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// ---- the restatement: what is true of each kind, one row per kind (kWaveH, kWave1, kWave2, kBlock, kBlockTall, kStream)
struct KindRule {
   int home;            // its side stream in a forked run
   bool alternates;     // it moves to the context's second wave stream on odd alternating runs
   int hold;            // microseconds it is always held in a forked run with holds
   int hold_if_tall;    // more when the tall kind runs too
   int hold_if_both;    // more when the tall AND the block kind run too
   bool yields_to_rest; // with wide rounds in a forked run it goes last and waits for every other kind
};
static const KindRule kRules[6] = {
   {0, true, 5, 0, 5, false}, {0, true, 5, 0, 5, false}, {0, true, 5, 0, 5, false},
   {2, false, 0, 5, 0, false}, {6, false, 0, 0, 0, false}, {1, false, 0, 0, 0, true}};

struct Expected {
   bool fork, wait_previous_run;
   unsigned split_runs;
   std::vector<sb::EmStep> steps;
};
static Expected by_rules(const sb::EmScheduleIn &in)
{
   Expected e;
   int n = 0;
   for (int k = 0; k < 6; ++k) n += in.present[k] ? 1 : 0;
   e.fork = n >= 2;
   e.wait_previous_run = in.split && in.per_run_state;
   const bool overlapping_runs = in.split && !in.per_run_state;  // the next run may start under this one
   const bool counts = overlapping_runs && e.fork && in.wave_alt > 0;
   e.split_runs = in.split_runs + (counts ? 1u : 0u);
   const bool odd_run = counts && in.split_runs % 2 == 1;
   std::vector<int> early, late;
   for (int k = 5; k >= 0; --k)
      if (in.present[k]) (e.fork && in.wide_rounds && kRules[k].yields_to_rest ? late : early).push_back(k);
   for (int pass = 0; pass < 2; ++pass)
      for (int k : pass ? late : early) {
         const KindRule &r = kRules[k];
         sb::EmStep st;
         st.kind = k;
         st.slot = e.fork ? (r.alternates && odd_run ? in.wave_alt : r.home) : -1;
         st.hold_us = 0;
         if (e.fork && !overlapping_runs)
            st.hold_us = r.hold + (in.present[sb::kBlockTall] ? r.hold_if_tall : 0) + (in.present[sb::kBlockTall] && in.present[sb::kBlock] ? r.hold_if_both : 0);
         st.after_others = pass == 1;
         e.steps.push_back(st);
      }
   return e;
}
static bool same(const sb::EmSchedule &s, const Expected &e)
{
   if (s.fork != e.fork || s.wait_previous_run != e.wait_previous_run || s.split_runs != e.split_runs || s.n_steps != (int)e.steps.size()) return false;
   for (int i = 0; i < s.n_steps; ++i)
      if (s.steps[i].kind != e.steps[(size_t)i].kind || s.steps[i].slot != e.steps[(size_t)i].slot || s.steps[i].hold_us != e.steps[(size_t)i].hold_us ||
          s.steps[i].after_others != e.steps[(size_t)i].after_others)
         return false;
   return true;
}

static sb::EmScheduleIn input(std::initializer_list<int> kinds, bool split, bool per_run_state, bool wide_rounds, int wave_alt, unsigned split_runs)
{
   sb::EmScheduleIn in;
   for (int k : kinds) in.present[k] = true;
   in.split = split, in.per_run_state = per_run_state, in.wide_rounds = wide_rounds, in.wave_alt = wave_alt, in.split_runs = split_runs;
   return in;
}
// one hand-written row: the steps as {kind, slot, hold_us, after_others}
static bool is(const sb::EmSchedule &s, bool fork, bool wait_previous_run, unsigned split_runs, std::vector<sb::EmStep> steps)
{
   return same(s, Expected{fork, wait_previous_run, split_runs, steps});
}

int main()
{
   using namespace sb;
   static_assert(kWaveH == 0 && kWave1 == 1 && kWave2 == 2 && kBlock == 3 && kBlockTall == 4 && kStream == 5 && kNumKinds == 6, "the rules' rows");
   CHECK(kAuxStreams == 8 && kBlockHoldUs == 5 && kWaveHoldUs == 5);
   for (int k = 0; k < 6; ++k) CHECK(kKindStream[k] == kRules[k].home && kKindStream[k] < kAuxStreams);
   // ---- every combination
   int n_cases = 0;
   for (int subset = 0; subset < 64; ++subset) {
      if (((subset & 1) + ((subset >> 1) & 1) + ((subset >> 2) & 1)) > 1) continue; // a plan uses one wave kind
      for (int split = 0; split < 2; ++split)
         for (int state = 0; state < 3; ++state) // no per-run state; phases only; wide rounds (which are per-run state)
            for (int wave_alt : {0, 3})
               for (unsigned runs = 0; runs < 4; ++runs) {
                  EmScheduleIn in;
                  for (int k = 0; k < 6; ++k) in.present[k] = (subset >> k) & 1;
                  in.split = split, in.per_run_state = state > 0, in.wide_rounds = state == 2, in.wave_alt = wave_alt, in.split_runs = runs;
                  const EmSchedule s = em_schedule(in);
                  if (!same(s, by_rules(in))) {
                     std::printf("kinds %#x split %d state %d wave_alt %d runs %u differ\n", subset, split, state, wave_alt, runs);
                     return 1;
                  }
                  for (int i = 0; i < s.n_steps; ++i) CHECK(s.steps[i].slot >= -1 && s.steps[i].slot < kAuxStreams && in.present[s.steps[i].kind]);
                  ++n_cases;
               }
   }
   CHECK(n_cases == 32 * 2 * 3 * 2 * 4);
   // ---- the schedules that matter, by hand
   // a wave kind alone: no fork, the caller's stream, no hold -- split or not
   CHECK(is(em_schedule(input({kWave1}, false, false, false, -1, 0)), false, false, 0, {{kWave1, -1, 0, false}}));
   CHECK(is(em_schedule(input({kWaveH}, true, false, false, 3, 1)), false, false, 1, {{kWaveH, -1, 0, false}}));
   // wave + block + tall, unsplit: tall, then block 5 us behind, then wave 10 us behind, on streams 6, 2, 0
   CHECK(is(em_schedule(input({kWave1, kBlock, kBlockTall}, false, false, false, -1, 0)), true, false, 0,
            {{kBlockTall, 6, 0, false}, {kBlock, 2, 5, false}, {kWave1, 0, 10, false}}));
   // without the tall kind nothing holds the block kind, and the wave kind waits 5 us only
   CHECK(is(em_schedule(input({kWave2, kBlock}, false, false, false, 3, 7)), true, false, 7, {{kBlock, 2, 0, false}, {kWave2, 0, 5, false}}));
   // the same three kinds in four consecutive split runs with a second wave stream: the wave kind alternates 0, 3, 0, 3, nothing is held
   unsigned runs = 0;
   for (int r = 0; r < 4; ++r) {
      const EmSchedule s = em_schedule(input({kWave1, kBlock, kBlockTall}, true, false, false, 3, runs));
      CHECK(is(s, true, false, (unsigned)r + 1, {{kBlockTall, 6, 0, false}, {kBlock, 2, 0, false}, {kWave1, r % 2 ? 3 : 0, 0, false}}));
      runs = s.split_runs;
   }
   CHECK(runs == 4);
   // ... and without one: stream 0 every time, and the counter stays
   CHECK(is(em_schedule(input({kWave1, kBlock, kBlockTall}, true, false, false, 0, 1)), true, false, 1,
            {{kBlockTall, 6, 0, false}, {kBlock, 2, 0, false}, {kWave1, 0, 0, false}}));
   // tile kinds + wide rounds, split: the run waits for the previous one, the stream kind goes last and waits for the others, the
   // holds are the unsplit ones, the wave kind stays on stream 0 and the counter stays (an odd one included)
   CHECK(is(em_schedule(input({kWave1, kBlock, kBlockTall, kStream}, true, true, true, 3, 1)), true, true, 1,
            {{kBlockTall, 6, 0, false}, {kBlock, 2, 5, false}, {kWave1, 0, 10, false}, {kStream, 1, 0, true}}));
   // the same unsplit: the stream kind still goes last; and without wide rounds (streaming fallback only) it goes first
   CHECK(is(em_schedule(input({kWave1, kBlock, kBlockTall, kStream}, false, true, true, -1, 0)), true, false, 0,
            {{kBlockTall, 6, 0, false}, {kBlock, 2, 5, false}, {kWave1, 0, 10, false}, {kStream, 1, 0, true}}));
   CHECK(is(em_schedule(input({kWave1, kBlock, kStream}, false, false, false, -1, 0)), true, false, 0,
            {{kStream, 1, 0, false}, {kBlock, 2, 0, false}, {kWave1, 0, 5, false}}));
   // wide rounds alone: one kind, no fork, nothing to wait behind -- but a split run still waits for the previous one
   CHECK(is(em_schedule(input({kStream}, true, true, true, 3, 0)), false, true, 0, {{kStream, -1, 0, false}}));
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("em_schedule_cpp")
    src, exe = d / "em_schedule.cpp", d / "em_schedule"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "strawberry_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_every_schedule_matches_the_rules_and_the_hand_written_rows(program):
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
