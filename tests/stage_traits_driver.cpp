// stage_traits_driver.cpp -- the table of sweep stages (csrc/pic_limits.h: stage_traits) and the coefficients the step schedule
// (csrc/host_schedule.h) hands a re-deriving sweep, as a stand-alone program for tests/test_stage_traits_cpu.py.  No input.
// stdout: one "T ..." per Stage 0 .. kStages - 1: the stage, the row's fields (arith rederives stores first second), then what
// follows from them (gathers reads_v pushes reads_tile leaves_tile wrap_only ends_step carries_solve profile_kind);
// then three planned calls, a refresh and seven plain Yoshida-4 steps on a large state: "C <readonly_c> <alternate_stores>" and
// one "L <stage> <c_prev> <d_prev>" per launch of the call (solves included).
#include <cstdio>

#include "host_plan.h"
#include "host_schedule.h"

int main() {
  for (int s = 0; s < kStages; ++s) {
    const StageTraits t = stage_traits(s);
    std::printf("T %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", s, (int)t.arith, (int)t.rederives, (int)t.stores, (int)t.first,
                (int)t.second, (int)gathers(t), (int)reads_v(t), (int)pushes(t), (int)reads_tile(t),
                (int)leaves_tile(t), (int)wrap_only(t), (int)ends_step(t), (int)carries_solve(t), profile_kind(t));
  }
  double cs[4], ds[4];
  yoshida_coefficients(cs, ds);
  const int modes[3][2] = {{1, 1}, {1, 0}, {0, 0}};
  for (const auto& m : modes) {
    Schedule S;
    CallShape p;
    p.cs = cs; p.ds = ds;
    p.light_inner_steps = true; p.readonly_c = m[0] != 0; p.alternate_stores = m[1] != 0;
    plan_refresh(S, p.scheme, [](const Launch&) {});
    std::printf("C %d %d\n", m[0], m[1]);
    plan_call(S, p, 7, [](const Launch& l) { std::printf("L %d %a %a\n", l.stage, l.c_prev, l.d_prev); });
  }
  return 0;
}
