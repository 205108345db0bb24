// pool_driver.cpp -- the layout of the pooled features' work block and the launch plan of their passes (csrc/host_blocks.h:
// pool_parts, pool_plan) as a stand-alone program, for tests/test_pool_cpu.py and tests/test_pool_ln_cpu.py.
// stdin: one call per line,  [ln] num_envs N H flags  (bit i of flags = field i of: per_env vjp host params_host xv g_x g_v
// g_params; a leading word "ln": the layer with a LayerNorm).
// stdout: one line each: "ok pool=<bytes>" followed by "view=<offset>" for each view in order ("null" for a part without
// elements).  The sizing pass (no base) must give the same bytes and set no view: the driver checks both.
// A line  plan num_envs N  gives "ok chunks_per_wg=<n> workgroups=<n>".
#include <cstdio>
#include <cstring>

#include "host_blocks.h"

static char* const BASE = reinterpret_cast<char*>(0x100000);

static void view(const char* name, const void* p) {
  if (p) std::printf(" %s=%td", name, static_cast<const char*>(p) - BASE);
  else std::printf(" %s=null", name);
}
#define VIEW(v, m) view(#m, (v).m)

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    long long E, N, H;
    int flags;
    if (std::sscanf(line, "plan %lld %lld", &E, &N) == 2) {
      const PoolPlan p = pool_plan((size_t)E, (size_t)N);
      std::printf("ok chunks_per_wg=%lld workgroups=%lld\n", p.chunks_per_wg, p.workgroups);
      continue;
    }
    const bool ln = std::strncmp(line, "ln ", 3) == 0;
    if (std::sscanf(line + (ln ? 3 : 0), "%lld %lld %lld %d", &E, &N, &H, &flags) != 4) {
      std::fprintf(stderr, "pool_driver: malformed line: %s", line);
      return 2;
    }
    BlockDims d;
    d.num_envs = (size_t)E;
    PoolCallShape s;
    s.N = (size_t)N; s.H = (size_t)H; s.ln = ln;
    bool* const flag[] = {&s.per_env, &s.vjp, &s.host, &s.params_host, &s.xv, &s.g_x, &s.g_v, &s.g_params};
    for (int i = 0; i < 8; ++i) *flag[i] = (flags >> i) & 1;
    PoolViews sized, v;
    const size_t want = pool_parts(Carver{}, d, s, sized);
    const size_t bytes = pool_parts(Carver{BASE}, d, s, v);
    if (want != bytes || sized.max || sized.acc || sized.gE || sized.params || sized.x || sized.g) {
      std::fprintf(stderr, "pool_driver: the sizing pass disagrees with the carving pass\n");
      return 3;
    }
    std::printf("ok pool=%zu", bytes);
    VIEW(v, max); VIEW(v, acc); VIEW(v, gE); VIEW(v, params); VIEW(v, x); VIEW(v, v); VIEW(v, cot); VIEW(v, out); VIEW(v, g_x);
    VIEW(v, g_v); VIEW(v, g);
    std::printf("\n");
  }
  return 0;
}
