// actor_driver.cpp -- the layout of the particle actor's call block (csrc/host_blocks.h: actor_parts) as a stand-alone program,
// for tests/test_actor_cpu.py.
// stdin: one call per line,  num_envs act_modes H P nsteps flags  (bit i of flags = field i of: per_env host stepping particles
// std noise features_out pre_out actions_out hist).
// stdout: one line each: "ok actor=<bytes>" followed by "view=<offset>" for each view in order ("null" for a part without
// elements).  The sizing pass (no base) must give the same bytes and set no view: the driver checks both.
#include <cstdio>

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
    long long E, M, H, P, T;
    int flags;
    if (std::sscanf(line, "%lld %lld %lld %lld %lld %d", &E, &M, &H, &P, &T, &flags) != 6) {
      std::fprintf(stderr, "actor_driver: malformed line: %s", line);
      return 2;
    }
    BlockDims d;
    d.num_envs = (size_t)E; d.act_modes = (size_t)M; d.P = (size_t)P;
    ActorCallShape s;
    s.H = (size_t)H; s.nsteps = (size_t)T;
    bool* const flag[] = {&d.per_env, &s.host, &s.stepping, &s.particles, &s.std, &s.noise, &s.features_out, &s.pre_out,
                          &s.actions_out, &s.hist};
    for (int i = 0; i < 10; ++i) *flag[i] = (flags >> i) & 1;
    ActorCallViews sized, v;
    const size_t want = actor_parts(Carver{}, d, s, sized);
    const size_t bytes = actor_parts(Carver{BASE}, d, s, v);
    if (want != bytes || sized.d_act || sized.d_feat || sized.d_hist || sized.d_params || sized.d_std || sized.d_noise ||
        sized.d_features || sized.d_pre_out) {
      std::fprintf(stderr, "actor_driver: the sizing pass disagrees with the carving pass\n");
      return 3;
    }
    std::printf("ok actor=%zu", bytes);
    VIEW(v, d_act); VIEW(v, d_feat); VIEW(v, d_hist); VIEW(v, d_params); VIEW(v, d_std); VIEW(v, d_noise); VIEW(v, d_features);
    VIEW(v, d_pre_out);
    std::printf("\n");
  }
  return 0;
}
