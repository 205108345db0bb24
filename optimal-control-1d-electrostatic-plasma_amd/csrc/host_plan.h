// host_plan.h -- the launch plan of a handle: everything pic_create derives from its pic_config and the device's CU count
// without touching the device.  No HIP in here: the header compiles with a plain host C++17 compiler, so that the plan of any
// configuration can be pinned on a CPU (tests/plan_driver.cpp, tests/test_plan_cpu.py).  A step's results do not depend on the
// launch geometry: no parity test notices a slip in these rules, it only costs speed.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "picstep.h"

#include "pic_limits.h"

enum Format : int { FMT_F64 = 0, FMT_F32 = 1, FMT_U32 = 2 };     // PosF64 / PosF32 / PosU32

struct LaunchPlan {
  int fmt = FMT_F64;
  int acc_kind = PIC_ACC_FIX64;  // resolved accumulator (never PIC_ACC_AUTO)
  int vec = 2;
  size_t esz = 8;          // particle element size (positions and velocities have the same width in every format)
  long long ld = 0;
  long long chunk = 0;
  int nblk = 0;
  int R = 1;
  int fg = 42;             // fractional bits of the fixed-point accumulators
  int S = 1;               // sub-rows per accumulator row (pic_device.h: acc_row_sum)
  double magic = 0;
  size_t sweep_lds = 0, solve_lds = 0;
  // resident schedule (pic_resident.h): one workgroup of res_nw waves holds an environment, res_ppt particles per lane
  bool resident = false;
  int res_ppt = 0, res_nw = 0, res_R = 1;
  bool res_lean = false;          // resident kernel without carried cell / weights (two workgroups per CU)
  size_t res_lds = 0;
  size_t res_carry_bytes = 0;     // the resident schedule's block of carried cells and weights (pic_resident.h: ResidentEdge); 0 = none
  double dx = 0, scale = 0;
  double cs[4]{}, ds[4]{};
  bool light_inner_steps = false;     // inner steps of a call end with sweep D2 (particle states of 256 MB and more)
  bool readonly_auto = false;         // whole steps run sweeps C_RO and D_RC / D2_RC unless pic_set_readonly_c says otherwise
  bool alternate_auto = false;        // ... and every second inner step of a call stores once unless pic_set_alternate_stores says otherwise
  size_t sweep_lds_rc = 0;            // LDS of the sweeps that re-derive another (D_RC, D2_RC, C_RB, B2_RD): sweep_lds and that sweep's field tile; 0 = does not fit
  bool v_separate = false;            // v is an allocation of its own (states of 256 MB and more: host_place.h, alloc_particles)
  bool h_part_at_create = false;      // pinned staging for x | v from pic_create on (states up to 4 MB)
  bool h_fields = false;              // pinned staging for n | E_mesh | phi (meshes up to 256 KB each in total)
};

static inline void yoshida_coefficients(double (&c)[4], double (&d)[4]) {
  // integration.py:62-69, same expressions in the same order
  const double cbrt2 = std::pow(2.0, 1.0 / 3.0);
  const double w0 = (-1) * cbrt2 / (2 - cbrt2);
  const double w1 = 1 / (2 - cbrt2);
  c[0] = c[3] = 0.5 * w1;
  c[1] = c[2] = 0.5 * (w0 + w1);
  d[0] = 0.0;
  d[1] = d[3] = w1;
  d[2] = w0;
}

static inline int plan_fail(std::string* err, const std::string& msg) {
  if (err) *err = msg;
  return PIC_EINVAL;
}

// the argument checks of pic_create that need no device
static inline int check_config(const pic_config& c, std::string* err) {
  const pic_config* cfg = &c;
  if (cfg->N < 1 || cfg->Ng < 4 || cfg->num_envs < 1 || !(cfg->L > 0) || !(cfg->dt > 0) || !(cfg->n0 > 0))
    return plan_fail(err, "pic_create: need N>=1, Ng>=4, num_envs>=1, L>0, dt>0, n0>0");
  if (cfg->N > (1ll << 36)) return plan_fail(err, "pic_create: N > 2^36");
  if (cfg->num_envs > 65535) return plan_fail(err, "pic_create: num_envs > 65535");
  if (cfg->env_index_base < 0) return plan_fail(err, "pic_create: env_index_base < 0");
  if (cfg->particle_dtype != PIC_F64 && cfg->particle_dtype != PIC_F32)
    return plan_fail(err, "pic_create: particle_dtype must be PIC_F64 or PIC_F32");
  if (cfg->position_dtype != PIC_POS_FLOAT && cfg->position_dtype != PIC_POS_FIXED32)
    return plan_fail(err, "pic_create: position_dtype must be PIC_POS_FLOAT or PIC_POS_FIXED32");
  if (cfg->position_dtype == PIC_POS_FIXED32 && cfg->particle_dtype != PIC_F32)
    return plan_fail(err, "pic_create: 32-bit fixed-point positions go with float32 particles");
  if (cfg->accum_dtype < PIC_ACC_AUTO || cfg->accum_dtype > PIC_ACC_F64)
    return plan_fail(err, "pic_create: accum_dtype must be PIC_ACC_AUTO, _FIX64, _PACKED or _F64");
  if (cfg->interpol != PIC_CIC && cfg->interpol != PIC_TSC)
    return plan_fail(err, "pic_create: interpol must be PIC_CIC or PIC_TSC");
  if (cfg->accum_dtype == PIC_ACC_PACKED && cfg->particle_dtype != PIC_F32)
    return plan_fail(err, "pic_create: the packed accumulator needs float32 particles");
  if (cfg->accum_dtype == PIC_ACC_PACKED && cfg->interpol != PIC_CIC)
    return plan_fail(err, "pic_create: the packed accumulator is CIC only");
  if (cfg->placement != PIC_PLACE_AUTO && cfg->placement != PIC_PLACE_OFF)
    return plan_fail(err, "pic_create: placement must be PIC_PLACE_AUTO or PIC_PLACE_OFF");
  if (cfg->placement_ms < 0) return plan_fail(err, "pic_create: placement_ms < 0");
  if (cfg->accum_dtype == PIC_ACC_F64 && cfg->particle_dtype != PIC_F64)
    return plan_fail(err, "pic_create: the float64 accumulator needs float64 particles");
  return PIC_OK;
}

// The plan of `c` on a device of ncu compute units.  c has passed check_config.
static inline int plan_launch(const pic_config& c, int ncu, LaunchPlan* p, std::string* err) {
  const pic_config* cfg = &c;
  *p = LaunchPlan{};
  p->fmt = cfg->particle_dtype == PIC_F64 ? FMT_F64 : (cfg->position_dtype == PIC_POS_FIXED32 ? FMT_U32 : FMT_F32);
  p->acc_kind = cfg->accum_dtype;
  if (p->acc_kind == PIC_ACC_AUTO)
    p->acc_kind = (cfg->particle_dtype == PIC_F32 && cfg->interpol == PIC_CIC) ? PIC_ACC_PACKED : PIC_ACC_FIX64;
  p->esz = cfg->particle_dtype == PIC_F64 ? 8 : 4;
  p->vec = cfg->particle_dtype == PIC_F64 ? 2 : 4;
  p->dx = cfg->L / cfg->Ng;                                   // pic.py:36
  p->scale = cfg->n0 * cfg->L / (double)cfg->N / p->dx;       // interpolate.py:18
  yoshida_coefficients(p->cs, p->ds);
  p->ld = (cfg->N + 63) / 64 * 64;
  // fixed-point accumulators: the weights of all N particles on one node must fit in 63 bits
  int lg = 0;
  while ((1ll << lg) < cfg->N + 1) ++lg;
  p->fg = 62 - lg > 50 ? 50 : 62 - lg;
  p->magic = std::ldexp(1.5, 52 - p->fg);
  {  // to_fixed (pic_device.h) subtracts the high words alone: the low word of magic's bit pattern is zero for every fg
    std::uint64_t bits;
    std::memcpy(&bits, &p->magic, sizeof(bits));
    if ((bits & 0xffffffffull) != 0) return plan_fail(err, "pic_create: the fixed-point magic has a non-zero low word");
  }

  // workgroups per environment: enough in total to fill 256 CUs several times, at least one
  // BLOCK*VEC tile each
  const long long tile = (long long)BLOCK * p->vec;
  long long nblk = cfg->blocks_per_env;      // workgroups per environment of the streaming sweeps (resets and probes always use them)
  if (nblk <= 0) {
    const long long target_total = 8192;      // ~128 workgroups per env at 64 envs (profiles/experiments_r1.md)
    nblk = (target_total + cfg->num_envs - 1) / cfg->num_envs;
    // Large environments: >= 8 tiles per workgroup (amortises the prologue and the flush).  Small ones in small
    // ensembles are latency-bound (profiles/experiments_r2.md: N = 1e5 13 -> 98 workgroups 47 -> 28 us/step; N = 1e6
    // is best at 122 whatever the number of environments): one tile per workgroup, at most 64 workgroups per environment.
    const bool small = (double)cfg->N * cfg->num_envs <= 4.0e6 && cfg->N <= 131072;
    long long tiles_min = small ? 1 : 8;
    // one or two large environments: 4 tiles per workgroup, so that there is a workgroup for every CU (N = 1e6, one
    // environment: 122 workgroups 64 us/step, 245 56 us, 489 63 us)
    if (!small && (cfg->N + 8 * tile - 1) / (8 * tile) * cfg->num_envs < 256) tiles_min = 4;
    long long max_by_work = (cfg->N + tiles_min * tile - 1) / (tiles_min * tile);
    if (small && max_by_work > 64) max_by_work = 64;
    if (nblk > max_by_work) nblk = max_by_work;
    if (nblk < 1) nblk = 1;
    // ... and at most ~10 tiles (80 KB of x, 80 KB of v) per workgroup: a total of 8192 workgroups is 156 000 particles each at
    // config 5's share -- 340 us per workgroup, and a last partial round of workgroups that long at the end of every sweep.  Scans
    // of both large shares (profiles/bpe_big.sh): N = 4e6 x 64 float64 128 -> 384 workgroups per environment 4078 -> 3997 us per
    // step (512: 4029), N = 1e7 x 128 float32 64 -> 512: 10223 -> 9913 (768: 9928, 1024: 10058); config 2 (122) is not touched.
    const long long by10 = (cfg->N + 10 * tile - 1) / (10 * tile);
    if (!small && nblk < by10) nblk = by10;
    // A handful of large environments run as one to six workgroups per CU: a total that fills the CUs unevenly leaves some
    // with one workgroup more than others for the whole sweep (3 x 1e6: 3 x 123 = 369 workgroups on 256 CUs 63.3 us/step, 3 x 163
    // = 489 58.9).  Take the workgroups per environment from the smallest k >= 2 workgroups per CU that keeps >= 8 tiles' worth
    // ... per workgroup where it can (k ncu / E, at most the 4-tile count); 1, 2, 4, 6, 8, 12 environments keep what they had.
    if (!small) {
      const long long by4 = (cfg->N + 4 * tile - 1) / (4 * tile);
      if (nblk * cfg->num_envs < 6ll * ncu) {
        for (long long k = 2; k <= 6; ++k) {
          long long c = k * ncu / cfg->num_envs;
          if (c > by4) c = by4;
          if (c >= nblk || c == by4) { nblk = c; break; }
        }
      }
    }
  }
  {                                          // a workgroup's chunk of x or v is addressed with 31-bit byte offsets (StreamOut)
    const long long cap = (1ll << 27) - tile;
    if (nblk < (cfg->N + cap - 1) / cap) nblk = (cfg->N + cap - 1) / cap;
  }
  if (p->acc_kind == PIC_ACC_PACKED) {       // count field of the packed accumulator: < 2^20 particles per workgroup
    const long long cap = (1ll << 20) - tile;
    if (nblk < (cfg->N + cap - 1) / cap) nblk = (cfg->N + cap - 1) / cap;
  }
  long long chunk = (cfg->N + nblk - 1) / nblk;
  chunk = (chunk + tile - 1) / tile * tile;
  nblk = (cfg->N + chunk - 1) / chunk;
  if (nblk > 65535) return plan_fail(err, "pic_create: blocks_per_env too large");
  p->chunk = chunk;
  p->nblk = (int)nblk;
  // Sub-rows of an accumulator row (pic_device.h: acc_row_sum): with few environments all workgroups of an environment flush
  // at about the same time, and their atomics on one 8 Ng-byte row are serialised at the memory side.  At most 4 sub-rows (1 / 2 /
  // 3 / 4 environments of 1e6: 31.2 / 45.0 / 64.5 / 74.0 us per step with 4, 31.6 / 45.3 / 65.5 / 75.1 with 8, 33.3 / 47.8 /
  // 65.2 / 75.4 with 16: every reader sums them), at least 8 workgroups per sub-row; with 16 environments or more the rows
  // themselves spread the traffic (and the flushes hide under the streaming of the other workgroups).
  // Inner steps of a multi-step call leave the deposit of their final positions to the next step's sweep B2 (host_schedule.h) where the
  // sweeps are bound by HBM -- a particle state that does not fit the 256 MB Infinity Cache: there sweep B has the issue slots that
  // sweep D lacks (config 2 969 -> 948 us per step).  States that live in the cache, or are bound by the latency of each launch,
  // gain nothing or lose (all measured on one box, round 3's tree against this one: 8 x 1e6 float64 131.2 -> 132.6, 64 x 20000
  // float32 TSC 26.2 -> 27.2, config 1 14.5 -> 14.7, one environment of N = 1e5 19.1 -> 19.4): they keep the full sweep D.
  p->light_inner_steps = 2.0 * (double)cfg->num_envs * (double)p->ld * (double)p->esz >= 256.0 * 1048576.0;
  // Whole steps on such a state also leave sweep C's stores out: sweep D re-derives C's output from C's input (ST_C_RO, ST_D_RC,
  // ST_D2_RC) -- 80 instead of 96 bytes per float64 particle-step, and D's extra sub-stage fits its issue slots with the wave-uniform
  // wrap (config 2 959 -> 865 us per step; profiles/r5_readonly.md).  pic_set_readonly_c overrides the choice.
  p->readonly_auto = p->light_inner_steps;
  p->S = 1;
  while (p->S < 4 && nblk / (2 * p->S) >= 8 && (long long)cfg->num_envs * 2 * p->S <= 32) p->S *= 2;

  const size_t stride = (size_t)cfg->Ng + 2;
  // LDS: 2 R meshes (sweep D deposits two) + the field tile.  R = 1: one mesh for the eight waves of a workgroup.  Copies per
  // wave pair (R = 4, rounds 1-2) bought nothing at config 2 and cost 2-4 % where a step is short (more to sum and clear per
  // workgroup); even with every particle in ONE cell a sweep is only 16 % slower, with 1 copy as with 4
  // (profiles/experiments_r2.md 17, profiles/clustered.py)
  p->R = 1;
  p->sweep_lds = 2 * p->R * stride * 8 + stride * p->esz;
  p->solve_lds = 2 * (size_t)cfg->Ng * sizeof(double);
  if (p->sweep_lds + stride * p->esz + kSweepStaticLds <= kLdsLimit) p->sweep_lds_rc = p->sweep_lds + stride * p->esz;
  else p->readonly_auto = false;
  // ... and store particles in every other sweep of a call's inner steps, not in two of three (host_schedule.h: X and Y steps;
  // 72 instead of 80 bytes per float64 particle-step; profiles/r8_alternate_stores.md)
  p->alternate_auto = p->readonly_auto;
  if (p->sweep_lds + kSweepStaticLds > kLdsLimit) {
    const long long max_ng = (long long)((kLdsLimit - kSweepStaticLds) / (2 * p->R * 8 + p->esz)) - 2;
    return plan_fail(err, "pic_create: Ng too large for the LDS-resident mesh (at most " + std::to_string(max_ng) +
                                     " cells with this particle dtype)");
  }
  // Resident schedule (pic_resident.h): environments whose particles fit one workgroup's registers are stepped by
  // one launch per pic_step call.  blocks_per_env: 0 = use it where it applies, > 0 = streaming sweeps with that many
  // workgroups, -1 = resident or fail.
  {
    // 512-thread workgroups holding 4, 8, 10 or 16 particles per lane (1024 threads leave 128 registers per lane:
    // the 10- and 16-particle bodies spill there, so larger environments stay with the sweeps)
    static const int shapes[4][3] = {{8, 4, 2048}, {8, 8, 4096}, {8, 10, 5120}, {8, 16, 8192}};
    for (const auto& sh : shapes)
      if (cfg->N <= sh[2]) { p->res_nw = sh[0]; p->res_ppt = sh[1]; break; }
    p->res_R = 1;   // one mesh per workgroup: replicas cost more in node sums and clearing than they save in LDS atomic contention (experiments_r2.md 17)
    auto need = [&](int R) { return (size_t)2 * R * stride * 8 + 4 * (size_t)cfg->Ng * 8 + stride * p->esz; };
    while (p->res_R > 1 && need(p->res_R) > 48 * 1024) p->res_R >>= 1;
    p->res_lds = need(p->res_R);
    const bool possible = p->res_nw != 0 && p->res_lds + kResidentStaticLds <= kLdsLimit && p->acc_kind != PIC_ACC_F64;
    if (cfg->blocks_per_env < 0 && !possible) {
      const long long max_ng = (long long)((kLdsLimit - kResidentStaticLds - 2 * (2 * 8 + p->esz)) / (2 * 8 + p->esz + 4 * 8));
      return plan_fail(err, "pic_create: the resident schedule needs N <= 8192, Ng <= " + std::to_string(max_ng) +
                                       " (this particle dtype) and an integer accumulator");
    }
    // Measured (profiles/experiments_r2.md): one workgroup steps 5000 float64 particles in ~17 us whatever the number of
    // environments, the sweeps need 22 us for one environment of 8000 and 35-110 us for 64-1024 of 5000.  A lone
    // large-ish environment is therefore left to the sweeps (they spread it over many CUs).
    const bool worth = cfg->N <= 5120 || cfg->num_envs >= 32;
    p->resident = possible && (cfg->blocks_per_env < 0 || (cfg->blocks_per_env == 0 && worth));
    // (carrying three TSC weights for 16 particles per lane would need more than 256 registers)
    p->res_lean = (cfg->num_envs > ncu && p->res_ppt <= 10) || (cfg->interpol == PIC_TSC && p->res_ppt == 16);
  }
  // what pic_create allocates beside the meshes
  if (p->resident && !p->res_lean && p->res_ppt <= 10 && p->esz == 8 && cfg->num_envs <= 32)
    p->res_carry_bytes = (size_t)cfg->num_envs * p->res_nw * 64 * p->res_ppt * (sizeof(int) + (cfg->interpol == PIC_TSC ? 4 : 2) * p->esz);
  p->v_separate = 2 * ((size_t)cfg->num_envs * p->ld * p->esz) >= ((size_t)256 << 20) && cfg->placement != PIC_PLACE_OFF;
  p->h_part_at_create = 2 * (size_t)cfg->num_envs * cfg->N * p->esz <= ((size_t)4 << 20);
  p->h_fields = (size_t)cfg->num_envs * cfg->Ng * sizeof(double) <= ((size_t)256 << 10);
  return PIC_OK;
}
