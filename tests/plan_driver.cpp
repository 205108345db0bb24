// plan_driver.cpp -- the launch planner (csrc/host_plan.h) as a stand-alone program, for tests/test_plan_cpu.py.
// stdin: one configuration per line,
//   N Ng num_envs particle_dtype position_dtype accum_dtype interpol blocks_per_env placement placement_ms env_index_base L dt n0 ncu
// stdout: one line each, "err <code> <message>" or "ok" and every LaunchPlan field as name=value (floating point as hex floats).
#include <cinttypes>
#include <cstdio>

#include "host_plan.h"

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    pic_config c{};
    long long N = 0;
    int ncu = 0;
    if (std::sscanf(line, "%lld %d %d %d %d %d %d %d %d %d %d %lf %lf %lf %d", &N, &c.Ng, &c.num_envs, &c.particle_dtype, &c.position_dtype,
                    &c.accum_dtype, &c.interpol, &c.blocks_per_env, &c.placement, &c.placement_ms, &c.env_index_base, &c.L, &c.dt, &c.n0,
                    &ncu) != 15) {
      std::fprintf(stderr, "plan_driver: malformed line: %s", line);
      return 2;
    }
    c.N = N;
    std::string err;
    LaunchPlan p;
    int rc = check_config(c, &err);
    if (!rc) rc = plan_launch(c, ncu, &p, &err);
    if (rc) {
      std::printf("err %d %s\n", rc, err.c_str());
      continue;
    }
    std::printf("ok fmt=%d acc_kind=%d esz=%zu vec=%d dx=%a scale=%a", p.fmt, p.acc_kind, p.esz, p.vec, p.dx, p.scale);
    for (int i = 0; i < 4; ++i) std::printf(" cs%d=%a", i, p.cs[i]);
    for (int i = 0; i < 4; ++i) std::printf(" ds%d=%a", i, p.ds[i]);
    std::printf(" ld=%lld fg=%d magic=%a chunk=%lld nblk=%d S=%d R=%d sweep_lds=%zu sweep_lds_rc=%zu solve_lds=%zu light_inner_steps=%d"
                " readonly_auto=%d resident=%d res_nw=%d res_ppt=%d res_R=%d res_lean=%d res_lds=%zu res_carry_bytes=%zu"
                " h_part_at_create=%d h_fields=%d v_separate=%d\n",
                p.ld, p.fg, p.magic, p.chunk, p.nblk, p.S, p.R, p.sweep_lds, p.sweep_lds_rc, p.solve_lds, (int)p.light_inner_steps,
                (int)p.readonly_auto, (int)p.resident, p.res_nw, p.res_ppt, p.res_R, (int)p.res_lean, p.res_lds, p.res_carry_bytes,
                (int)p.h_part_at_create, (int)p.h_fields, (int)p.v_separate);
  }
  return 0;
}
