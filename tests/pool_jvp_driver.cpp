// pool_jvp_driver.cpp -- the layout of the pooled features' work block for a forward-mode call (csrc/host_blocks.h: pool_parts with
// jvp) as a stand-alone program, for tests/test_pool_jvp_cpu.py.  tests/pool_driver.cpp keeps the calls without jvp.
// stdin: one call per line,  [ln] num_envs N H flags K tflags  (bit i of flags = field i of: per_env host params_host xv; bit i of
// tflags = field i of: d_x d_v d_params; a leading word "ln": the layer with a LayerNorm).
// stdout: one line each: "ok pool=<bytes>" followed by "view=<offset>" for each view in order ("null" for a part without
// elements).  The sizing pass (no base) must give the same bytes and set no view: the driver checks both.
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
    int flags, K, tflags;
    const bool ln = std::strncmp(line, "ln ", 3) == 0;
    if (std::sscanf(line + (ln ? 3 : 0), "%lld %lld %lld %d %d %d", &E, &N, &H, &flags, &K, &tflags) != 6) {
      std::fprintf(stderr, "pool_jvp_driver: malformed line: %s", line);
      return 2;
    }
    BlockDims d;
    d.num_envs = (size_t)E;
    PoolCallShape s;
    s.N = (size_t)N; s.H = (size_t)H; s.ln = ln; s.jvp = true; s.K = K;
    bool* const flag[] = {&s.per_env, &s.host, &s.params_host, &s.xv};
    for (int i = 0; i < 4; ++i) *flag[i] = (flags >> i) & 1;
    bool* const tflag[] = {&s.d_x, &s.d_v, &s.d_params};
    for (int i = 0; i < 3; ++i) *tflag[i] = (tflags >> i) & 1;
    PoolViews sized, v;
    const size_t want = pool_parts(Carver{}, d, s, sized);
    const size_t bytes = pool_parts(Carver{BASE}, d, s, v);
    if (want != bytes || sized.max || sized.tmax || sized.acc || sized.params || sized.d_params || sized.x || sized.out || sized.d_x ||
        sized.d_v) {
      std::fprintf(stderr, "pool_jvp_driver: the sizing pass disagrees with the carving pass\n");
      return 3;
    }
    std::printf("ok pool=%zu", bytes);
    VIEW(v, max); VIEW(v, tmax); VIEW(v, acc); VIEW(v, gE); VIEW(v, params); VIEW(v, d_params); VIEW(v, x); VIEW(v, v); VIEW(v, cot);
    VIEW(v, out); VIEW(v, g_x); VIEW(v, g_v); VIEW(v, g); VIEW(v, d_x); VIEW(v, d_v);
    std::printf("\n");
  }
  return 0;
}
