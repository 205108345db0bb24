// pic_pool.h -- pooled particle features (include/picstep.h: pic_pool, pic_pool_vjp; pic_pool_jvp: 7t): per
// environment
//   out_k = (1/N) sum_i act(b_k + W_k0 cos q_i + W_k1 sin q_i + W_k2 u_i),   q_i = 2 pi x_i / L,  u_i = v_i v_scale
// its vector-Jacobian product and its directional derivatives, without an [N][H] array: a lane holds kPoolPerLane particles
// (cos, sin, u) in registers and walks the H rows of W, which are the same for every lane of the workgroup (scalar loads).  The
// sums over particles are 64-bit integer sums of terms rounded to nearest in a power-of-two unit that is known before the pass
// (pic_moments' pattern), so nothing depends on the order of the particles, the grid or the batch.  Off the step path: the
// kernels read x, v and write their own work block only.  Built with -ffp-contract=off: every product is rounded before its sum.
// The passes are written once, as bodies over a layer type (below: "the skeleton"): PoolPlain here, PoolLn in pic_pool_ln.h.
// A kernel is a body with its layer.
#pragma once
#include <climits>

#include "pic_moments.h"    // kMomInfBits, mom_max_bits; pic_v2d_a8 (rows that start on 8 bytes only: N odd)

namespace {

constexpr int kPoolMaxHidden = 256;
constexpr int POOL_BLOCK = 256;          // 4 waves: a workgroup's chunk is 1024 particles, so 5000 particles still make 5 workgroups
constexpr int kPoolTiles = 2;            // 16-byte tiles (2 particles each) a lane holds through one walk over k
constexpr int kPoolPerLane = 2 * kPoolTiles;
constexpr int kPoolSkip = INT_MIN;       // a unit word: nothing is deposited, the result is +0
constexpr int kPoolNan = INT_MIN + 1;    // ... the result is NaN
constexpr double kTwoPi = 6.283185307179586;

struct PoolArgs {
  const double* x;             // [env][ld] positions (not necessarily wrapped)
  const double* v;             // [env][ld]
  const double* params;        // W [H][3] row-major, then b [H] (pic_pool_ln: then gamma [H], beta [H])
  unsigned long long* umax;    // [env] bit pattern of max |u|, zero between calls
  unsigned long long* acc;     // [env][H] (forward) or [env][kSums][H] (VJP) integer sums, zero between calls
  long long env_params;        // doubles from one environment's parameters to the next (0: shared)
  long long N, ld;
  long long chunks_per_wg;     // chunks of POOL_BLOCK * kPoolTiles tiles per workgroup: a workgroup's range is contiguous
  double L, v_scale;
  int H, activation;
  int bitsN;                   // 2^bitsN >= N
};

struct PoolVjpArgs {
  const double* cot;           // [env][H]
  double* g_x;                 // [env][N] dense rows, overwritten; or null
  double* g_v;                 // the same
  int want_params;             // deposit the parameter sums into acc [env][kSums][H]
};

__device__ __forceinline__ bool pool_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }
__device__ __forceinline__ double pool_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ bool pool_on(int ue) { return ue != kPoolSkip && ue != kPoolNan; }      // a unit word that deposits

// exponent of the unit of sums of N terms bounded by `bound`: 2^e >= bound, unit 2^(e + bitsN - 61) (two bits of headroom in an
// int64: no overflow, whatever the data); kPoolSkip for a zero bound, kPoolNan for a non-finite one
__device__ __forceinline__ int pool_unit(double bound, int bitsN) {
  if (!pool_finite(bound)) return kPoolNan;
  if (!(bound > 0.0)) return kPoolSkip;
  return ilogb(bound) + 1 + bitsN - 61;
}

// wave_incl_scan's DPP steps on 64-bit integers (a masked-off or absent source adds 0); all 64 lanes must be active
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ long long dpp_add_i64(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(v >> 32), CTRL, ROW_MASK, 0xF, true);
  return v + (long long)(((unsigned long long)hi << 32) | lo);
}

// sum over the 64 lanes, the same value in every lane
__device__ __forceinline__ long long wave_sum_i64(long long v) {
  v = dpp_add_i64<0x111>(v);
  v = dpp_add_i64<0x112>(v);
  v = dpp_add_i64<0x114>(v);
  v = dpp_add_i64<0x118>(v);
  v = dpp_add_i64<0x142, 0xA>(v);
  v = dpp_add_i64<0x143, 0xC>(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), 63);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// tile t (particles 2t, 2t + 1) of a row; the odd last particle is read alone, so nothing beyond N is ever read
__device__ __forceinline__ pic_v2d pool_tile(const double* __restrict__ row, long long t, long long N) {
  pic_v2d r = {0.0, 0.0};
  if (2 * t + 1 < N) {
    const pic_v2d_a8 q = stream_load(reinterpret_cast<const pic_v2d_a8*>(row + 2 * t));
    r[0] = q[0]; r[1] = q[1];
  } else if (2 * t < N) {
    r[0] = row[2 * t];
  }
  return r;
}

// the tiles [t0, t1) of workgroup blockIdx.x
__device__ __forceinline__ void pool_range(const PoolArgs& a, long long& t0, long long& t1) {
  const long long ntiles = (a.N + 1) / 2, per = a.chunks_per_wg * POOL_BLOCK * kPoolTiles;
  t0 = (long long)blockIdx.x * per;
  t1 = t0 + per < ntiles ? t0 + per : ntiles;
}

// a lane's particles of the chunk that starts at tile tc: cos q, sin q, u and whether the slot holds a particle
struct PoolLane {
  double c[kPoolPerLane], s[kPoolPerLane], u[kPoolPerLane];
  bool on[kPoolPerLane];
};

__device__ __forceinline__ void pool_load(const PoolArgs& a, const double* __restrict__ xe, const double* __restrict__ ve,
                                          long long tc, long long t1, PoolLane& p) {
#pragma unroll
  for (int j = 0; j < kPoolTiles; ++j) {
    const long long t = tc + (long long)j * POOL_BLOCK + threadIdx.x;
    const bool have = t < t1;
    const pic_v2d xt = have ? pool_tile(xe, t, a.N) : pic_v2d{0.0, 0.0};
    const pic_v2d vt = have ? pool_tile(ve, t, a.N) : pic_v2d{0.0, 0.0};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int s = 2 * j + m;
      const double q = (kTwoPi * xt[m]) / a.L;
      p.on[s] = have && 2 * t + m < a.N;
      sincos(q, &p.s[s], &p.c[s]);
      p.u[s] = vt[m] * a.v_scale;
    }
  }
}

// z_k = b_k, + W_k0 c, + W_k1 s, + W_k2 u: each product rounded, then the sum
__device__ __forceinline__ double pool_pre(double w0, double w1, double w2, double bk, double c, double s, double u) {
  double z = bk;
  z = z + w0 * c;
  z = z + w1 * s;
  z = z + w2 * u;
  return z;
}

// the activation of the argument z
__device__ __forceinline__ double pool_act(double z, bool is_tanh) { return is_tanh ? tanh(z) : (z > 0.0 ? z : 0.0); }

// (cot_k act'(z)) / N of one term
__device__ __forceinline__ double pool_dn(double z, double cot, double Nd, bool is_tanh) {
  double act;
  if (is_tanh) {
    const double h = tanh(z);
    act = 1.0 - h * h;
  } else {
    act = z > 0.0 ? 1.0 : 0.0;
  }
  return (cot * act) / Nd;
}

// ---- forward mode (pic_pool_jvp, pic_pool_ln_jvp) ---------------------------------------------------------------
constexpr int kPoolMaxDirs = 8;                      // directions of one call
constexpr double kPoolJvpUp = 0x1.0000000001p+0;     // 1 + 2^-40: above the rounding of the JVP's bounds and terms

struct PoolJvpArgs {
  const double* d_x;           // [K][env][N] dense rows, or null: 0
  const double* d_v;           // the same
  const double* d_params;      // [K][P] or [K][env][P] in the parameters' layout, or null: 0
  unsigned long long* tmax;    // [2][K][env] bit patterns of max |tq|, max |tu|; zero between calls
  long long dir_params;        // doubles from one direction's tangent parameters to the next
  int K, num_envs;
};

// what the bounds of one (direction, environment) rest on: u_max, tq_max, tu_max
struct PoolJvpMax { double umx, tqm, tum; };
// ... and what a layer adds per (direction, environment): Z_max and r_max (the LayerNorm's)
struct PoolJvpEnv { PoolJvpMax m; double zmax, rmx; };

// a lane's tangents of a group of KD directions: tq = ((2 pi) d_x) / L and tu = d_v v_scale of its particles
template <int KD>
struct PoolTan { double tq[KD][kPoolPerLane], tu[KD][kPoolPerLane]; };

// the direction's max words of an environment; false where one is saturated (a non-finite tq or tu: that direction is NaN)
__device__ __forceinline__ bool pool_jvp_max(const PoolJvpArgs& t, int dir, int env, double umx, PoolJvpMax& m) {
  const unsigned long long qb = t.tmax[((size_t)0 * t.K + dir) * t.num_envs + env];
  const unsigned long long ub = t.tmax[((size_t)1 * t.K + dir) * t.num_envs + env];
  m = PoolJvpMax{umx, __longlong_as_double((long long)qb), __longlong_as_double((long long)ub)};
  return qb < kMomInfBits && ub < kMomInfBits;
}

// the direction's tangent parameters of an environment (null: 0)
__device__ __forceinline__ const double* pool_jvp_params(const PoolArgs& a, const PoolJvpArgs& t, int dir, int env) {
  return t.d_params ? t.d_params + (size_t)dir * t.dir_params + (size_t)env * a.env_params : nullptr;
}

// Z_k, the bound of |dz_ik|: |db_k|, + |dW_k0|, + |dW_k1|, + |dW_k2| u_max, + (|W_k0| + |W_k1|) tq_max, + |W_k2| tu_max
template <typename TRow>
__device__ __forceinline__ double pool_jvp_z(double w0, double w1, double w2, const TRow& d, const PoolJvpMax& m) {
  double Z = fabs(d.b);
  Z = Z + fabs(d.w0);
  Z = Z + fabs(d.w1);
  Z = Z + fabs(d.w2) * m.umx;
  Z = Z + (fabs(w0) + fabs(w1)) * m.tqm;
  Z = Z + fabs(w2) * m.tum;
  return Z;
}

// dz_ik = db_k, + dW_k0 c, + dW_k1 s, + dW_k2 u, + (W_k1 c - W_k0 s) tq, + W_k2 tu: each product rounded, then the sum
template <typename TRow>
__device__ __forceinline__ double pool_dz(double w0, double w1, double w2, const TRow& d, double c, double s, double u, double tq,
                                          double tu) {
  double dz = d.b;
  dz = dz + d.w0 * c;
  dz = dz + d.w1 * s;
  dz = dz + d.w2 * u;
  dz = dz + (w1 * c - w0 * s) * tq;
  dz = dz + w2 * tu;
  return dz;
}

// a_ik: the activation's derivative at the argument z
__device__ __forceinline__ double pool_dact(double z, bool is_tanh) {
  if (is_tanh) {
    const double h = tanh(z);
    return 1.0 - h * h;
  }
  return z > 0.0 ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------------
// The plain layer (pic_pool, pic_pool_vjp).  What a layer type supplies to the skeleton below:
//   kSums, kUnits          the VJP's parameter sums and unit words per hidden unit
//   Row, row(k)            the parameters of unit k (the same for every lane: scalar loads)
//   Stats, prepare()       what a lane's particles need before a walk over k
//   arg()                  the activation's argument of particle j under unit k (and y_ik where there is one)
//   env_bad()              whether the environment is NaN as a whole apart from its particles; the same in every thread
//   fwd_unit()             the unit word of out_k
//   vjp_env(), vjp_units(), vjp_unit()   the VJP's per-environment values, the unit words of unit k into LDS, that of sum m
//   first_walk(), back()   what the VJP does before its walk, and d cost / d z_ik from (cot_k act') / N
//   clear()                the layer's own max words of an environment, behind the finish
//   kRmax, trow(), jvp_env(), jvp_unit()   forward mode: whether the max pass takes r_max, the tangent row of unit k, the
//                          (direction, environment)'s values, the unit word of d_out_k
//   Tan, jvp_walks(), jvp_dn()   ... what a lane's particles need per direction before the walk, and dn_ik from dz_ik
// ---------------------------------------------------------------------------------------------
struct PoolPlain {
  static constexpr int kSums = 4, kUnits = 1;      // r c, r s, r u, r in one unit
  static constexpr bool kRmax = false;
  struct Row { double w0, w1, w2, b; };
  struct Stats {};
  const double* __restrict__ p;
  int H, activation, bitsN;

  __device__ __forceinline__ PoolPlain(const PoolArgs& a, int env)
      : p(a.params + (size_t)env * a.env_params), H(a.H), activation(a.activation), bitsN(a.bitsN) {}
  __device__ __forceinline__ Row row(int k) const { return Row{p[3 * k], p[3 * k + 1], p[3 * k + 2], p[3 * H + k]}; }
  __device__ __forceinline__ static bool row_finite(const Row& w) {
    return pool_finite(w.w0) && pool_finite(w.w1) && pool_finite(w.w2) && pool_finite(w.b);
  }
  __device__ __forceinline__ bool env_bad(const double*, double) const { return false; }
  __device__ __forceinline__ void prepare(const PoolLane&, Stats&) const {}
  __device__ __forceinline__ double arg(const Row& w, const PoolLane& q, const Stats&, int j, double& y) const {
    y = 0.0;
    return pool_pre(w.w0, w.w1, w.w2, w.b, q.c[j], q.s[j], q.u[j]);
  }
  // tanh is bounded by 1 = 2^0; relu by B_k = |W_k0| + |W_k1| + |W_k2| u_max + |b_k|, rounded up
  __device__ __forceinline__ int fwd_unit(int k, double umx) const {
    const Row w = row(k);
    if (!row_finite(w)) return kPoolNan;
    if (activation == PIC_ACT_TANH) return bitsN - 61;
    const double B = ((fabs(w.w0) + fabs(w.w1)) + fabs(w.w2) * umx) + fabs(w.b);
    return pool_unit(B * 0x1.0000000000004p+0, bitsN);     // (1 + 2^-50: above the rounding of B and of z)
  }
  __device__ __forceinline__ void vjp_env(const double*, double, int) {}
  // the unit word of g_W_k*, g_b_k (every m): every term is bounded by (|g_k| / N) max(1, u_max)
  __device__ __forceinline__ int vjp_unit(int, int k, double gk, double umx, double Nd) const {
    if (!row_finite(row(k))) return kPoolNan;
    return pool_unit((fabs(gk) / Nd) * (umx > 1.0 ? umx : 1.0), bitsN);
  }
  __device__ __forceinline__ void vjp_units(int* unit, int k, double gk, double umx, double Nd, bool dep) const {
    unit[k] = dep ? vjp_unit(0, k, gk, umx, Nd) : kPoolSkip;
  }
  __device__ __forceinline__ void first_walk(const PoolLane&, Stats&, const double*, double, bool, const int*,
                                             unsigned long long*) const {}
  __device__ __forceinline__ double back(const Row&, double dn, double, const Stats&, int) const { return dn; }
  __device__ __forceinline__ void clear(int) const {}

  // forward mode (pic_pool_jvp): the tangent row of unit k (tp: the direction's tangent parameters, null = 0), nothing per
  // environment or per particle, the unit word of d_out_k from the bound Z_k, and dn = dz
  template <int KD> struct Tan {};
  __device__ __forceinline__ static Row trow(const double* __restrict__ tp, int H, int k) {
    return tp ? Row{tp[3 * k], tp[3 * k + 1], tp[3 * k + 2], tp[3 * H + k]} : Row{0.0, 0.0, 0.0, 0.0};
  }
  __device__ __forceinline__ PoolJvpEnv jvp_env(const double*, const PoolJvpMax& m, int) const { return PoolJvpEnv{m, 0.0, 0.0}; }
  __device__ __forceinline__ int jvp_unit(int k, const double* __restrict__ tp, const PoolJvpEnv& e) const {
    const Row w = row(k);
    if (!row_finite(w)) return kPoolNan;
    return pool_unit(pool_jvp_z(w.w0, w.w1, w.w2, trow(tp, H, k), e.m) * kPoolJvpUp, bitsN);
  }
  template <int KD>
  __device__ __forceinline__ void jvp_walks(const PoolLane&, const Stats&, const PoolTan<KD>&, const double* const (&)[KD],
                                            const bool (&)[KD], Tan<KD>&) const {}
  template <int KD>
  __device__ __forceinline__ double jvp_dn(const Row&, const Row&, double dz, double, const Stats&, const Tan<KD>&, int, int) const {
    return dz;
  }
};

// ---------------------------------------------------------------------------------------------
// The skeleton: the four passes of either layer
// ---------------------------------------------------------------------------------------------
// Per-environment max |u| as the bit pattern of a non-negative double into umax[env] (zero before).  A non-finite u or q
// saturates it at kMomInfBits: the finishing kernels then write NaN for that environment.  Grid: the passes'.
__global__ __launch_bounds__(POOL_BLOCK) void pool_max_kernel(PoolArgs a) {
  const int env = blockIdx.y;
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  long long t0, t1;
  pool_range(a, t0, t1);
  unsigned long long mb = 0ull;
  for (long long t = t0 + threadIdx.x; t < t1; t += POOL_BLOCK) {
    const pic_v2d xt = pool_tile(xe, t, a.N), vt = pool_tile(ve, t, a.N);     // (a slot beyond N holds 0)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      mom_max_bits(mb, fabs(vt[m] * a.v_scale));
      if (!pool_finite((kTwoPi * xt[m]) / a.L)) mb = kMomInfBits;
    }
  }
  block_max_to(__longlong_as_double((long long)mb), a.umax + env);
}

// Forward pass: grid (workgroups per environment, environments).  LDS: the H unit words and H 64-bit sums.  Per chunk a lane
// computes cos, sin and u of its particles once (and what the layer prepares from them), then for every k its kPoolPerLane
// terms, rounded to integers; the wave's sum (DPP) is one ds_add_u64 per wave and k.  The flush is one memory-side atomic per
// non-zero k into acc [env][H].
template <typename Layer>
__device__ __forceinline__ void pool_fwd_body(const PoolArgs& a, const Layer& layer) {
  __shared__ unsigned long long sums[kPoolMaxHidden];
  __shared__ int unit[kPoolMaxHidden];
  const int env = blockIdx.y, H = a.H, lane = threadIdx.x & 63;
  const unsigned long long mb = a.umax[env];
  if (mb >= kMomInfBits) return;                           // (uniform: the finishing kernel writes NaN)
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  const double umx = __longlong_as_double((long long)mb);
  if (layer.env_bad(nullptr, umx)) return;                 // (uniform, the same)
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    sums[k] = 0ull;
    unit[k] = layer.fwd_unit(k, umx);
  }
  __syncthreads();
  long long t0, t1;
  pool_range(a, t0, t1);
  const bool is_tanh = a.activation == PIC_ACT_TANH;
  for (long long tc = t0; tc < t1; tc += (long long)POOL_BLOCK * kPoolTiles) {
    PoolLane q;
    pool_load(a, xe, ve, tc, t1, q);
    typename Layer::Stats st;
    layer.prepare(q, st);
    for (int k = 0; k < H; ++k) {
      const int ue = unit[k];
      if (!pool_on(ue)) continue;                          // (uniform)
      const typename Layer::Row w = layer.row(k);
      long long part = 0;
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        double y;
        const double h = pool_act(layer.arg(w, q, st, j, y), is_tanh);
        if (q.on[j]) part += __double2ll_rn(ldexp(h, -ue));
      }
      part = wave_sum_i64(part);
      if (lane == 0 && part) atomicAdd(sums + k, (unsigned long long)part);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    const unsigned long long s = sums[k];
    if (s) atomicAdd(a.acc + (size_t)env * H + k, s);
  }
}

// One workgroup per environment: the integer sums to out [env][H] = sum / N; +0 where nothing was deposited, NaN in the outputs
// of a unit whose word is kPoolNan and in every output of an environment that is NaN as a whole (a non-finite particle, or the
// layer's rule); the accumulators and the environment's max word are cleared behind the read.
template <typename Layer>
__device__ __forceinline__ void pool_finish_body(const PoolArgs& a, const Layer& layer, double* __restrict__ out) {
  const int env = blockIdx.x, H = a.H;
  const unsigned long long mb = a.umax[env];
  const bool finite = mb < kMomInfBits;
  const double umx = finite ? __longlong_as_double((long long)mb) : 0.0;
  const bool bad = layer.env_bad(nullptr, umx) || !finite;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    unsigned long long* s = a.acc + (size_t)env * H + k;
    const int ue = bad ? kPoolNan : layer.fwd_unit(k, umx);
    double r = 0.0;
    if (ue == kPoolNan) r = pool_nan();
    else if (ue != kPoolSkip) r = ldexp((double)(long long)*s, ue) / (double)a.N;
    out[(size_t)env * H + k] = r;
    *s = 0ull;
  }
  __syncthreads();                                         // (every lane has read the max word)
  if (threadIdx.x == 0) a.umax[env] = 0ull;
}

// The vector-Jacobian product for a cotangent g.cot [env][H]: the forward's pass with the activations recomputed.  One thread
// owns a particle, so g_x_i and g_v_i are float64 sums over ascending k; the parameter terms dz c, dz s, dz u, dz
// (dz_ik = d cost / d z_ik: the layer's `back`) are rounded to integers in the unit of k and summed like the forward's.  What
// the layer deposits besides is its `first_walk`'s.  An environment that is NaN as a whole gets NaN rows and deposits nothing:
// the finishing kernel writes the parameters' NaN.  LDS: kSums H sums and kUnits H unit words.
template <typename Layer>
__device__ __forceinline__ void pool_vjp_body(const PoolArgs& a, const PoolVjpArgs& g, Layer& layer) {
  __shared__ unsigned long long sums[Layer::kSums * kPoolMaxHidden];
  __shared__ int unit[Layer::kUnits * kPoolMaxHidden];
  const int env = blockIdx.y, H = a.H, lane = threadIdx.x & 63;
  const unsigned long long mb = a.umax[env];
  const bool finite = mb < kMomInfBits;
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  const double* __restrict__ ge = g.cot + (size_t)env * H;
  const double umx = finite ? __longlong_as_double((long long)mb) : 0.0, Nd = (double)a.N;
  const bool bad = layer.env_bad(ge, umx) || !finite;
  layer.vjp_env(ge, Nd, env);
  long long t0, t1;
  pool_range(a, t0, t1);
  if (bad) {                                               // (uniform)
    const long long i1 = 2 * t1 < a.N ? 2 * t1 : a.N;
    for (long long i = 2 * t0 + threadIdx.x; i < i1; i += POOL_BLOCK) {
      if (g.g_x) g.g_x[(size_t)env * a.N + i] = pool_nan();
      if (g.g_v) g.g_v[(size_t)env * a.N + i] = pool_nan();
    }
    return;
  }
  const bool dep = g.want_params != 0;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
#pragma unroll
    for (int m = 0; m < Layer::kSums; ++m) sums[m * H + k] = 0ull;
    layer.vjp_units(unit, k, ge[k], umx, Nd, dep);
  }
  __syncthreads();
  const bool is_tanh = a.activation == PIC_ACT_TANH;
  const double cx = kTwoPi / a.L;
  for (long long tc = t0; tc < t1; tc += (long long)POOL_BLOCK * kPoolTiles) {
    PoolLane q;
    pool_load(a, xe, ve, tc, t1, q);
    typename Layer::Stats st;
    layer.prepare(q, st);
    layer.first_walk(q, st, ge, Nd, is_tanh, unit, sums);
    double sx[kPoolPerLane], sv[kPoolPerLane];
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) sx[j] = sv[j] = 0.0;
    for (int k = 0; k < H; ++k) {
      const int ue = unit[k];
      const bool on = pool_on(ue);                         // (uniform)
      const typename Layer::Row w = layer.row(k);
      const double gk = ge[k];
      long long pc = 0, ps = 0, pu = 0, pr = 0;
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        double y;
        const double z = layer.arg(w, q, st, j, y);
        const double r = layer.back(w, pool_dn(z, gk, Nd, is_tanh), y, st, j);
        sx[j] = sx[j] + r * (w.w1 * q.c[j] - w.w0 * q.s[j]);
        sv[j] = sv[j] + r * w.w2;
        if (on && q.on[j]) {
          pc += __double2ll_rn(ldexp(r * q.c[j], -ue));
          ps += __double2ll_rn(ldexp(r * q.s[j], -ue));
          pu += __double2ll_rn(ldexp(r * q.u[j], -ue));
          pr += __double2ll_rn(ldexp(r, -ue));
        }
      }
      if (on) {
        pc = wave_sum_i64(pc);
        ps = wave_sum_i64(ps);
        pu = wave_sum_i64(pu);
        pr = wave_sum_i64(pr);
        if (lane == 0) {
          if (pc) atomicAdd(sums + k, (unsigned long long)pc);
          if (ps) atomicAdd(sums + H + k, (unsigned long long)ps);
          if (pu) atomicAdd(sums + 2 * H + k, (unsigned long long)pu);
          if (pr) atomicAdd(sums + 3 * H + k, (unsigned long long)pr);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) {
      if (!q.on[j]) continue;
      const long long i = 2 * (tc + (long long)(j >> 1) * POOL_BLOCK + threadIdx.x) + (j & 1);
      const size_t o = (size_t)env * a.N + i;
      if (g.g_x) g.g_x[o] = cx * sx[j];
      if (g.g_v) g.g_v[o] = a.v_scale * sv[j];
    }
  }
  __syncthreads();
  if (!dep) return;
  for (int c = threadIdx.x; c < Layer::kSums * H; c += POOL_BLOCK) {
    const unsigned long long s = sums[c];
    if (s) atomicAdd(a.acc + (size_t)env * Layer::kSums * H + c, s);
  }
}

// One workgroup per environment: the kSums H integer sums to gE [env][kSums H] in the parameters' order (g_W [H][3], then [H]
// each); +0 where the bound is zero, NaN for a non-finite bound and for an environment that is NaN as a whole; the accumulators
// and the max words are cleared behind the read.
template <typename Layer>
__device__ __forceinline__ void pool_vjp_finish_body(const PoolArgs& a, const PoolVjpArgs& g, Layer& layer, double* __restrict__ gE) {
  const int env = blockIdx.x, H = a.H, P = Layer::kSums * H;
  const unsigned long long mb = a.umax[env];
  const bool finite = mb < kMomInfBits;
  const double* __restrict__ ge = g.cot + (size_t)env * H;
  const double umx = finite ? __longlong_as_double((long long)mb) : 0.0, Nd = (double)a.N;
  const bool bad = layer.env_bad(ge, umx) || !finite;
  layer.vjp_env(ge, Nd, env);
  if (g.want_params) {
    for (int c = threadIdx.x; c < P; c += POOL_BLOCK) {
      const int m = c / H, k = c - m * H;
      unsigned long long* s = a.acc + (size_t)env * P + c;
      const int ue = bad ? kPoolNan : layer.vjp_unit(m, k, ge[k], umx, Nd);
      double r = 0.0;
      if (ue == kPoolNan) r = pool_nan();
      else if (ue != kPoolSkip) r = ldexp((double)(long long)*s, ue);
      gE[(size_t)env * P + (m < 3 ? 3 * k + m : m * H + k)] = r;
      *s = 0ull;
    }
  }
  __syncthreads();                                         // (every lane has read the max words)
  if (threadIdx.x == 0) {
    a.umax[env] = 0ull;
    layer.clear(env);
  }
}

// The forward mode's max pass: pool_max_kernel's word (the LayerNorm's: and r_max, as pool_ln_max_kernel) and, per direction,
// the largest |tq_i| and |tu_i| of the environment as bit patterns into t.tmax (a non-finite one saturates its word: that
// direction of that environment is NaN).  x, v and every direction's d_x, d_v are read once.  Grid: the passes'.
template <typename Layer>
__device__ __forceinline__ void pool_jvp_max_body(const PoolArgs& a, const PoolJvpArgs& t, const Layer& layer,
                                                  unsigned long long* __restrict__ rmax) {
  const int env = blockIdx.y;
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  long long t0, t1;
  pool_range(a, t0, t1);
  unsigned long long mb = 0ull, rb = 0ull, qb[kPoolMaxDirs], ub[kPoolMaxDirs];
#pragma unroll
  for (int d = 0; d < kPoolMaxDirs; ++d) qb[d] = ub[d] = 0ull;
  for (long long tc = t0; tc < t1; tc += (long long)POOL_BLOCK * kPoolTiles) {
    if constexpr (Layer::kRmax) {
      PoolLane q;
      pool_load(a, xe, ve, tc, t1, q);
      typename Layer::Stats st;
      layer.prepare(q, st);
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        if (!q.on[j]) continue;
        mom_max_bits(mb, fabs(q.u[j]));
        if (!pool_finite(q.c[j])) mb = kMomInfBits;        // (cos of a non-finite q is NaN)
        mom_max_bits(rb, st.r[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kPoolTiles; ++j) {
      const long long tt = tc + (long long)j * POOL_BLOCK + threadIdx.x;
      if (tt >= t1) continue;
      if constexpr (!Layer::kRmax) {
        const pic_v2d xt = pool_tile(xe, tt, a.N), vt = pool_tile(ve, tt, a.N);     // (a slot beyond N holds 0)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          mom_max_bits(mb, fabs(vt[m] * a.v_scale));
          if (!pool_finite((kTwoPi * xt[m]) / a.L)) mb = kMomInfBits;
        }
      }
#pragma unroll
      for (int d = 0; d < kPoolMaxDirs; ++d) {
        if (d >= t.K) continue;                            // (uniform)
        const size_t row = ((size_t)d * t.num_envs + env) * a.N;
        const pic_v2d dx = t.d_x ? pool_tile(t.d_x + row, tt, a.N) : pic_v2d{0.0, 0.0};
        const pic_v2d dv = t.d_v ? pool_tile(t.d_v + row, tt, a.N) : pic_v2d{0.0, 0.0};
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          mom_max_bits(qb[d], fabs((kTwoPi * dx[m]) / a.L));
          mom_max_bits(ub[d], fabs(dv[m] * a.v_scale));
        }
      }
    }
  }
  block_max_to(__longlong_as_double((long long)mb), a.umax + env);
  if constexpr (Layer::kRmax) block_max_to(__longlong_as_double((long long)rb), rmax + env);
#pragma unroll
  for (int d = 0; d < kPoolMaxDirs; ++d) {
    if (d >= t.K) continue;
    block_max_to(__longlong_as_double((long long)qb[d]), t.tmax + ((size_t)0 * t.K + d) * t.num_envs + env);
    block_max_to(__longlong_as_double((long long)ub[d]), t.tmax + ((size_t)1 * t.K + d) * t.num_envs + env);
  }
}

// The forward mode's pass: grid (workgroups per environment, environments, groups of KD directions).  The forward's pass with
// the activation's derivative in place of the activation: cos, sin, u, the layer's statistics and a_ik are computed once per
// particle (and k) and serve every direction of the group, whose tangents tq, tu a lane keeps in registers.  Per k and
// direction the term a_ik dn_ik (dn from dz: the layer's) is rounded to an integer in the unit of that (direction, k) and
// summed like the forward's.  LDS: KD H unit words and sums.  A direction that is NaN as a whole deposits nothing.
template <typename Layer, int KD>
__device__ __forceinline__ void pool_jvp_body(const PoolArgs& a, const PoolJvpArgs& t, const Layer& layer) {
  __shared__ unsigned long long sums[KD * kPoolMaxHidden];
  __shared__ int unit[KD * kPoolMaxHidden];
  const int env = blockIdx.y, H = a.H, lane = threadIdx.x & 63, d0 = blockIdx.z * KD;
  const unsigned long long mb = a.umax[env];
  if (mb >= kMomInfBits) return;                           // (uniform: the finishing kernel writes NaN)
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  const double umx = __longlong_as_double((long long)mb);
  if (layer.env_bad(nullptr, umx)) return;                 // (uniform, the same)
  const double* tp[KD];
  bool live[KD];
  bool any = false;
#pragma unroll
  for (int d = 0; d < KD; ++d) {                           // (everything here is uniform)
    const int dir = d0 + d;
    PoolJvpMax m{umx, 0.0, 0.0};
    live[d] = dir < t.K && pool_jvp_max(t, dir, env, umx, m);
    tp[d] = live[d] ? pool_jvp_params(a, t, dir, env) : nullptr;
    const PoolJvpEnv e = layer.jvp_env(tp[d], m, env);     // (every thread: it may hold barriers)
    for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
      sums[d * H + k] = 0ull;
      unit[d * H + k] = live[d] ? layer.jvp_unit(k, tp[d], e) : kPoolSkip;
    }
    any = any || live[d];
  }
  if (!any) return;
  __syncthreads();
  long long t0, t1;
  pool_range(a, t0, t1);
  const bool is_tanh = a.activation == PIC_ACT_TANH;
  for (long long tc = t0; tc < t1; tc += (long long)POOL_BLOCK * kPoolTiles) {
    PoolLane q;
    pool_load(a, xe, ve, tc, t1, q);
    typename Layer::Stats st;
    layer.prepare(q, st);
    PoolTan<KD> tn;
#pragma unroll
    for (int d = 0; d < KD; ++d) {
      const size_t row = ((size_t)(d0 + d) * t.num_envs + env) * a.N;
#pragma unroll
      for (int j = 0; j < kPoolTiles; ++j) {
        const long long tt = tc + (long long)j * POOL_BLOCK + threadIdx.x;
        const bool have = live[d] && tt < t1;
        const pic_v2d dx = have && t.d_x ? pool_tile(t.d_x + row, tt, a.N) : pic_v2d{0.0, 0.0};
        const pic_v2d dv = have && t.d_v ? pool_tile(t.d_v + row, tt, a.N) : pic_v2d{0.0, 0.0};
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          tn.tq[d][2 * j + m] = (kTwoPi * dx[m]) / a.L;
          tn.tu[d][2 * j + m] = dv[m] * a.v_scale;
        }
      }
    }
    typename Layer::template Tan<KD> lt;
    layer.template jvp_walks<KD>(q, st, tn, tp, live, lt);
    for (int k = 0; k < H; ++k) {
      int ue[KD];
      bool on = false;
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        ue[d] = unit[d * H + k];
        on = on || pool_on(ue[d]);
      }
      if (!on) continue;                                   // (uniform)
      const typename Layer::Row w = layer.row(k);
      typename Layer::Row tw[KD];
      long long part[KD];
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        tw[d] = Layer::trow(tp[d], H, k);
        part[d] = 0;
      }
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        double y;
        const double act = pool_dact(layer.arg(w, q, st, j, y), is_tanh);
#pragma unroll
        for (int d = 0; d < KD; ++d) {
          if (!pool_on(ue[d])) continue;                   // (uniform)
          const double dz = pool_dz(w.w0, w.w1, w.w2, tw[d], q.c[j], q.s[j], q.u[j], tn.tq[d][j], tn.tu[d][j]);
          const double term = act * layer.template jvp_dn<KD>(w, tw[d], dz, y, st, lt, d, j);
          if (q.on[j]) part[d] += __double2ll_rn(ldexp(term, -ue[d]));
        }
      }
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        if (!pool_on(ue[d])) continue;
        const long long s = wave_sum_i64(part[d]);
        if (lane == 0 && s) atomicAdd(sums + d * H + k, (unsigned long long)s);
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < KD * H; c += POOL_BLOCK) {
    const int d = c / H, k = c - d * H;
    const unsigned long long s = sums[c];
    if (s) atomicAdd(a.acc + ((size_t)(d0 + d) * t.num_envs + env) * H + k, s);      // (a direction beyond K deposited nothing)
  }
}

// One workgroup per environment, direction after direction: the integer sums to d_out [K][env][H] = sum / N; +0 where the
// bound is zero, NaN for a unit word kPoolNan, for a direction whose tq or tu is not finite and for an environment that is NaN
// as a whole; the accumulators and every max word of the environment are cleared behind the read.
template <typename Layer>
__device__ __forceinline__ void pool_jvp_finish_body(const PoolArgs& a, const PoolJvpArgs& t, const Layer& layer,
                                                     double* __restrict__ d_out) {
  const int env = blockIdx.x, H = a.H;
  const unsigned long long mb = a.umax[env];
  const bool finite = mb < kMomInfBits;
  const double umx = finite ? __longlong_as_double((long long)mb) : 0.0;
  const bool bad = layer.env_bad(nullptr, umx) || !finite;
  for (int dir = 0; dir < t.K; ++dir) {
    PoolJvpMax m;
    const bool live = pool_jvp_max(t, dir, env, umx, m) && !bad;
    if (!live) m = PoolJvpMax{umx, 0.0, 0.0};
    const double* __restrict__ tp = pool_jvp_params(a, t, dir, env);
    const PoolJvpEnv e = layer.jvp_env(tp, m, env);
    for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
      const size_t o = ((size_t)dir * t.num_envs + env) * H + k;
      const int ue = live ? layer.jvp_unit(k, tp, e) : kPoolNan;
      double r = 0.0;
      if (ue == kPoolNan) r = pool_nan();
      else if (ue != kPoolSkip) r = ldexp((double)(long long)a.acc[o], ue) / (double)a.N;
      d_out[o] = r;
      a.acc[o] = 0ull;
    }
  }
  __syncthreads();                                         // (every lane has read the max words)
  if (threadIdx.x == 0) {
    a.umax[env] = 0ull;
    layer.clear(env);
  }
  for (int c = threadIdx.x; c < 2 * t.K; c += POOL_BLOCK) t.tmax[(size_t)c * t.num_envs + env] = 0ull;
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_kernel(PoolArgs a) { pool_fwd_body(a, PoolPlain(a, blockIdx.y)); }

__global__ __launch_bounds__(POOL_BLOCK) void pool_finish_kernel(PoolArgs a, double* __restrict__ out) {
  pool_finish_body(a, PoolPlain(a, blockIdx.x), out);
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_vjp_kernel(PoolArgs a, PoolVjpArgs g) {
  PoolPlain layer(a, blockIdx.y);
  pool_vjp_body(a, g, layer);
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_vjp_finish_kernel(PoolArgs a, PoolVjpArgs g, double* __restrict__ gE) {
  PoolPlain layer(a, blockIdx.x);
  pool_vjp_finish_body(a, g, layer, gE);
}

constexpr int kPoolJvpDirs = 4;          // directions of a group of pool_jvp_kernel (the largest without scratch)

__global__ __launch_bounds__(POOL_BLOCK) void pool_jvp_max_kernel(PoolArgs a, PoolJvpArgs t) {
  pool_jvp_max_body(a, t, PoolPlain(a, blockIdx.y), nullptr);
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_jvp_kernel(PoolArgs a, PoolJvpArgs t) {
  pool_jvp_body<PoolPlain, kPoolJvpDirs>(a, t, PoolPlain(a, blockIdx.y));
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_jvp_finish_kernel(PoolArgs a, PoolJvpArgs t, double* __restrict__ d_out) {
  pool_jvp_finish_body(a, t, PoolPlain(a, blockIdx.x), d_out);
}

}  // namespace
