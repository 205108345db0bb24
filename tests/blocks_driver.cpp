// blocks_driver.cpp -- the layouts of the carved device blocks (csrc/host_blocks.h) as a stand-alone program, for
// tests/test_blocks_cpu.py.
// stdin: one shape per line,
//   num_envs ld Ng act_modes max_steps every K obs_walk nx nv feq_per_env P obs_modes per_env chunks nsteps flags
// (K: directions; obs_walk: the tangent walk's observed modes; P, obs_modes, per_env: the policy's; chunks: the phase JVP's;
// nsteps: a policy call's; flags: bit i set = field i of FLAGS below, what a policy call gives and wants).
// stdout: one line each: for every layout "name=<bytes>" followed by "view=<offset>" for each of its views in order ("null" for a
// part without elements).
#include <cinttypes>
#include <cstdio>

#include "host_blocks.h"

// the members of the kernels' argument blocks that tangent_parts and moments_jvp_parts fill (pic_tangent.h: TanArgs,
// pic_moments.h: MomJvpArgs)
struct TanHolder {
  double *st = nullptr, *dF = nullptr;
  long long *acc = nullptr, *ke = nullptr;
  unsigned long long* umax = nullptr;
};
struct MomJvpHolder {
  unsigned long long *acc = nullptr, *umax = nullptr;
};

static char* const BASE = reinterpret_cast<char*>(0x100000);

static void head(const char* name, size_t bytes) { std::printf(" %s=%zu", name, bytes); }
static void view(const char* name, const void* p) {
  if (p) std::printf(" %s=%td", name, static_cast<const char*>(p) - BASE);
  else std::printf(" %s=null", name);
}
#define VIEW(v, m) view(#m, (v).m)

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    long long E, ld, Ng, M, T, every, P, Mo, chunks, nsteps;
    int K, mo, nx, nv, fpe, per_env, flags;
    if (std::sscanf(line, "%lld %lld %lld %lld %lld %lld %d %d %d %d %d %lld %lld %d %lld %lld %d", &E, &ld, &Ng, &M, &T, &every, &K, &mo, &nx,
                    &nv, &fpe, &P, &Mo, &per_env, &chunks, &nsteps, &flags) != 17) {
      std::fprintf(stderr, "blocks_driver: malformed line: %s", line);
      return 2;
    }
    BlockDims d;
    d.num_envs = (size_t)E; d.ld = (size_t)ld; d.Ng = (size_t)Ng; d.act_modes = (size_t)M;
    d.P = (size_t)P; d.obs_modes = (size_t)Mo; d.per_env = per_env != 0; d.chunks = (size_t)chunks;
    PolicyCallShape s;             // FLAGS, bit 0 upwards:
    s.nsteps = (size_t)nsteps;
    bool* const flag[] = {&s.host, &s.stepping, &s.scale, &s.std, &s.noise, &s.obs, &s.pre, &s.obs_out, &s.pre_out, &s.actions_out,
                          &s.hist, &s.d_params, &s.d_obs, &s.d_pre};
    for (int i = 0; i < 14; ++i) *flag[i] = (flags >> i) & 1;
    const Carver c{BASE};
    std::printf("ok");
    { TapeViews v; head("tape", tape_parts(c, d, T, every, v));
      VIEW(v, ck); VIEW(v, ext); VIEW(v, seg); VIEW(v, F); VIEW(v, M); VIEW(v, lam); VIEW(v, cot); VIEW(v, gext); VIEW(v, nu); VIEW(v, acc);
      VIEW(v, cmax); VIEW(v, gact); }
    { LawViews v; head("law", law_parts(c, d, T, v)); VIEW(v, act); VIEW(v, modes); VIEW(v, cot); VIEW(v, E); }
    { KlViews v; head("kl", tape_kl_parts(c, d, nx, nv, fpe != 0, T, v)); VIEW(v, feq); VIEW(v, acc); VIEW(v, g); VIEW(v, trace); VIEW(v, cot); }
    { MomCotViews v; head("mom_cot", tape_moments_parts(c, d, T, v)); VIEW(v, cot); }
    { MomTraceViews v; head("mom_trace", tape_moments_trace_parts(c, d, T, v)); VIEW(v, trace); }
    { TapePolicyViews v; head("tape_policy", tape_policy_parts(c, d, T, v));
      VIEW(v, obs); VIEW(v, pre); VIEW(v, act); VIEW(v, gobs); VIEW(v, gpre); VIEW(v, gact); VIEW(v, cobs); VIEW(v, cact); VIEW(v, mbar);
      VIEW(v, gE); VIEW(v, g); }
    { PolicyCopyViews v; head("policy_copy", policy_copy_parts(c, d, s.scale, v)); VIEW(v, params); VIEW(v, scale); }
    { TanHolder v; head("tangent", tangent_parts(c, d, K, v)); VIEW(v, st); VIEW(v, dF); VIEW(v, acc); VIEW(v, ke); VIEW(v, umax); }
    { TanKlViews v; head("tangent_kl", tangent_kl_parts(c, d, K, v)); VIEW(v, ones); VIEW(v, part); }
    { MomViews v; head("moments", moments_parts(c, d, v)); VIEW(v, acc); VIEW(v, max); VIEW(v, out); }
    { MomJvpHolder v; head("moments_jvp", moments_jvp_parts(c, d, K, v)); VIEW(v, acc); VIEW(v, umax); }
    { TanWalkViews v; head("tanwalk", tanwalk_parts(c, d, K, mo, v));
      VIEW(v, dM); VIEW(v, hist); VIEW(v, obs); VIEW(v, dm); VIEW(v, da); VIEW(v, dG); VIEW(v, in); }
    { TanPolViews v; head("tanpol", tanpol_parts(c, d, K, v)); VIEW(v, dtheta); VIEW(v, du); VIEW(v, pin); }
    { PolicyCallViews v; head("policy", policy_parts(c, d, s, v));
      VIEW(v, d_act); VIEW(v, d_hist); VIEW(v, d_params); VIEW(v, d_scale); VIEW(v, d_std); VIEW(v, d_noise); VIEW(v, d_obs);
      VIEW(v, d_obs_out); VIEW(v, d_pre_out); }
    { PolicyVjpViews v; head("policy_vjp", policy_vjp_parts(c, d, s, v));
      VIEW(v, gE); VIEW(v, g); VIEW(v, params); VIEW(v, scale); VIEW(v, obs); VIEW(v, pre); VIEW(v, cot); VIEW(v, g_obs); VIEW(v, g_pre); }
    { PolicyJvpViews v; head("policy_jvp", policy_jvp_parts(c, d, s, K, v));
      VIEW(v, params); VIEW(v, scale); VIEW(v, obs); VIEW(v, pre); VIEW(v, d_params); VIEW(v, d_obs); VIEW(v, d_pre); VIEW(v, du); VIEW(v, da); }
    std::printf("\n");
  }
  return 0;
}
