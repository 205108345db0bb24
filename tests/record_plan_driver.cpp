// record_plan_driver.cpp -- the plan of the rollout recorder's particle pass (csrc/host_blocks.h: record_plan) as a stand-alone
// program, for tests/test_record_edges_cpu.py.
// stdin: one call per line,  plan N vec E xb vb px pv  (particles, particles per 16-byte tile, environments, marginal bins,
// phase bins).
// stdout: one line each: "ok gx=<n> tiles_per_wg=<n> rr=<n> phase_lds=<0|1> lds=<bytes>".
#include <cstdio>

#include "host_blocks.h"

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    long long N, vec;
    int E, xb, vb, px, pv;
    if (std::sscanf(line, "plan %lld %lld %d %d %d %d %d", &N, &vec, &E, &xb, &vb, &px, &pv) != 7) {
      std::fprintf(stderr, "record_plan_driver: malformed line: %s", line);
      return 2;
    }
    const RecordPlan p = record_plan(N, vec, E, xb, vb, px, pv);
    std::printf("ok gx=%d tiles_per_wg=%lld rr=%d phase_lds=%d lds=%zu\n", p.gx, p.tiles_per_wg, p.rr, p.phase_lds, p.lds);
  }
  return 0;
}
