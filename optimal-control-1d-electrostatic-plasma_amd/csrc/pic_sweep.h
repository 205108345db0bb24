// pic_sweep.h -- the push sweeps: in-prologue field solve, one particle through one Yoshida sub-stage, flush of the
// LDS mesh into the global fixed-point accumulators, and sweep_kernel<P, A, SHAPE, STAGE> itself; the stages of
// the other integrators (push_scheme).
#pragma once
#include "pic_device.h"
#include "pic_solve.h"

namespace {

// Field tile of a sweep workgroup, computed in its own prologue from the accumulator row the previous sweep
// filled: density -> b = n - n0 -> G = dx cumsum(b) - mean -> E_j = -(G_{j+1/2} + G_{j-1/2})/2 (+ E_ext).
// Every workgroup of an environment repeats the solve (2 KB of input at Ng = 256, read through L2); in exchange a
// step has no field-solve launch between its sweeps.  sb: Ng doubles of LDS scratch.
// ctl (pointers of THIS environment): the external field on the mesh, or the actuator coefficients it is built from here
// (xt: Ng doubles of LDS scratch for it) -- a controlled step has no actuator launch either.
// first: the deposit of node threadIdx.x, requested by the caller BEFORE its particle tile (the solve is what the workgroup
// waits for first, and a wave's loads return in the order they were issued); it is waited for here, behind the actuator product
template <typename T, int OFF>
__device__ __forceinline__ void prologue_field(const acc_t* __restrict__ acc_in, const AccRequest& first, int S, long long sub,
                                               const Control& ctl, double* __restrict__ ext_out, int Ng, double unit, double scale,
                                               double n0, double dx, double* __restrict__ sb, double* __restrict__ xt,
                                               double* __restrict__ slot, T* __restrict__ Es) {
  const int tid = threadIdx.x;
  if (ctl.act)
    for (int j = tid; j < Ng; j += BLOCK) {
      const double e = actuator_field(ctl.basis, ctl.basis + (size_t)Ng * ctl.M, ctl.act, j, ctl.M);   // actuator.py:54-63
      xt[j] = e;
      if (ext_out) ext_out[j] = e;
    }
  if (tid < Ng) sb[tid] = ((double)acc_row_finish(first, S) * unit) * scale - n0;           // interpolate.py:16-18, pic.py:116
  for (int j = tid + BLOCK; j < Ng; j += BLOCK)
    sb[j] = ((double)acc_row_sum(acc_in, j, S, sub) * unit) * scale - n0;
  __syncthreads();
  PIC_STAMP(3);
  scan_fields(sb, nullptr, Ng, dx, slot);
  __syncthreads();
  PIC_STAMP(4);
  const double gmean = slot[0];
  for (int i = tid; i < Ng + 2; i += BLOCK) {
    int node = i - OFF;
    node = node < 0 ? node + Ng : (node >= Ng ? node - Ng : node);
    const double gp = sb[node] - gmean;
    const double gm = sb[node == 0 ? Ng - 1 : node - 1] - gmean;
    double E = -0.5 * (gp + gm);
    if (ctl.act) E += xt[node];                                                           // util.py:102-103
    else if (ctl.ext) E += ctl.ext[node];
    Es[i] = (T)E;
  }
  __syncthreads();
  PIC_STAMP(5);
}

// Does a `locate` of the sweeps fold the index Ng to node 0?  Behind wrap_periodic a position lies in [0, L) (or is parked at 0), so
// j = floor(xw / dx) lies in [0, Ng], and j == Ng happens where the quotient rounds up (L = 50: Ng = 150 and 300 at
// xw = nextafter(L, 0)).  A sweep's LDS meshes and field tiles have Ng + 2 slots; with CIC the prologue fills Es[Ng] = E[0] and
// Es[Ng + 1] = E[1], so a gather at j = Ng reads what the folded one reads, and a deposit at j = Ng lands in slots Ng and Ng + 1,
// which mesh_node_sum<.., WIDE> adds to nodes 0 and 1: the same integer sums, without a compare and a select per locate.  TSC
// uses both ghost slots for its own offset and the packed accumulator has one word per cell: they fold.  So does everything that
// does not come from a wrap (sweep B2's locate_in_box on stored positions) and every kernel outside this file.
template <typename A, int SHAPE>
constexpr bool kFoldIndex = !(SHAPE == PIC_CIC && !std::is_same<A, fix_t>::value);

// The force evaluation of one sub-stage: gather at q from the field tile Es, kick p with d, drift q with c.
template <typename P, int SHAPE, bool FOLD>
__device__ __forceinline__ void substage(typename P::X& q, typename P::V& p, const typename P::W* __restrict__ Es,
                                         typename P::W d, typename P::W c, const Consts<P>& k, unsigned& bad) {
  using T = typename P::W;
  T w[3];
  typename P::X xw;
  int j;
  unsigned frac;
  locate<P, SHAPE, FOLD>(q, k, xw, j, w, frac, bad);            // (behind a wrap: 0 <= j <= Ng, kFoldIndex)
  const T E = gather_field<T, SHAPE>(Es, j, w);                 // util.py:105 / pic.py:120
  p = p + (typename P::V)((d * (-E)) * k.dt);                   // integration.py:32, pic.py:127
  q = drift<P>(q, p, c, k, bad);                                // integration.py:42
}

// One particle through one sub-stage.  Stages D / REFRESH also deposit the NEXT step's first drift
// position q1 = x' + (c1 p) dt into a second mesh (acc2), which is exactly what sweep A of the next
// step would deposit from the stored x', p -- so that sweep (a full read of x and v) is skipped.
// A stage that does not store is the storing one here; the stage behind it first repeats what it did not store, from its field
// tile Es2 (stage_traits: rederives).  That repeated drift and locate count into a scratch counter: they were counted already.
template <typename P, typename A, int SHAPE, int STAGE>
__device__ __forceinline__ void push_one(typename P::X& xq, typename P::V& vp, const typename P::W* __restrict__ Es,
                                         const typename P::W* __restrict__ Es2, A* __restrict__ acc, A* __restrict__ acc2,
                                         const Consts<P>& k, double& ke, unsigned& bad) {
  constexpr StageTraits kT = stage_traits(STAGE);
  constexpr bool kFold = kFoldIndex<A, SHAPE>;           // every locate<.., kFold> below comes behind a wrap: 0 <= j <= Ng
  using T = typename P::W;
  T w[3];
  typename P::X xw;
  int j;
  unsigned frac;
  typename P::X q = xq;
  typename P::V p = vp;
  if (reads_tile(kT)) {                                  // the sub-stage of the sweep before, which did not store, from its tile Es2
    unsigned again = 0u;
    if (kT.rederives == AR_B) q = drift<P>(q, p, k.c_next, k, again);       // sweep B2_RO's drift on the stored x', v' first: q1 (c_next is c1 in every sweep)
    substage<P, SHAPE, kFold>(q, p, Es2, k.d_prev, k.c_prev, k, again);     // (q2, v1) behind sweeps B2_RO and C_RO, (q3, v2) behind D2_RO
    if constexpr (kT.rederives == AR_D && !P::kFixed) q = wrap_periodic(q, k.L, again);   // ... and sweep D2_RO's wrap: the x', v' it did not store
  }
  if (kT.second == M2_INPUT) {
    // The post-step deposit of the PREVIOUS step (pic.py:145): q is the x' that step's sweep D2 wrapped and stored, so cell and
    // weights are the ones its own deposit would have had (locate = wrap + locate_in_box, and the wrap of a wrapped position
    // is the position).  A value outside [0, L) cannot come from D2; should memory hold one, its index folds to node 0 below.
    if constexpr (P::kFixed) locate<P, SHAPE>(q, k, xw, j, w, frac, bad);
    else locate_in_box<P, SHAPE>(q, k, j, w, frac);               // (straight from memory, no wrap in front: folds)
    deposit<A, P, SHAPE>(acc2, j, w, frac, k.magic);
  }
  if (kT.arith == AR_A) {
    q = drift<P>(q, p, k.c_cur, k, bad);                          // integration.py:42, c1
  } else if (gathers(kT)) {
    // q1 again (it is never stored); ST_B2_RD's c_prev is the re-derived drift's, its c1 is c_next's -- the same double
    if (kT.arith == AR_B) q = drift<P>(q, p, kT.rederives == AR_D ? k.c_next : k.c_prev, k, bad);
    substage<P, SHAPE, kFold>(q, p, Es, k.d_cur, k.c_cur, k, bad);
  }
  if (wrap_only(kT)) {                                 // the wrap alone: the deposit of x' is the next sweep B2's
    if constexpr (P::kFixed) xw = q;
    else xw = wrap_periodic(q, k.L, bad);
  } else {
    locate<P, SHAPE, kFold>(q, k, xw, j, w, frac, bad);
    deposit<A, P, SHAPE>(acc, j, w, frac, k.magic);
  }
  if (kT.second == M2_NEXT_Q1) {
    q = xw;                                                       // pic.py:139 (+ util.py:51)
    ke += (double)p * (double)p;
    const typename P::X qn = drift<P>(q, p, k.c_next, k, bad);    // next step's q1 (integration.py:42, c1)
    typename P::X xn;
    locate<P, SHAPE, kFold>(qn, k, xn, j, w, frac, bad);
    deposit<A, P, SHAPE>(acc2, j, w, frac, k.magic);
  }
  xq = q;
  vp = p;
}

// One particle through a step of symplectic or forward Euler, or a sub-stage of Stormer-Verlet (ST_SE, ST_FE, ST_VK, ST_VM;
// integration.py:8-10, :26-58, pic_set_integrator).  Each starts from the field of the deposit of the position it reads, with
// push_one's operand order: kick p + (d (-E)) dt, drift q + (c p) dt.  The reference skips a kick or drift whose coefficient is
// zero; so do these (Verlet's closing half-kick has no drift at all).
template <typename P, typename A, int SHAPE, int STAGE>
__device__ __forceinline__ void push_scheme(typename P::X& xq, typename P::V& vp, const typename P::W* __restrict__ Es,
                                            A* __restrict__ acc, const Consts<P>& k, double& ke, unsigned& bad) {
  using T = typename P::W;
  using V = typename P::V;
  T w[3];
  typename P::X xw;
  int j;
  unsigned frac;
  typename P::X q = xq;
  V p = vp;
  constexpr bool kFold = kFoldIndex<A, SHAPE>;                  // (both locates come behind a wrap: 0 <= j <= Ng)
  locate<P, SHAPE, kFold>(q, k, xw, j, w, frac, bad);
  const T E = gather_field<T, SHAPE>(Es, j, w);                 // util.py:105 / pic.py:120
  if (STAGE == ST_FE) {
    // integration.py:10, eta + dt grad(eta): the drift takes the velocity the step starts with.  (grad_func has wrapped eta's
    // positions in place, util.py:51; the stored x is wrapped already, so xw is q)
    q = drift<P>(xw, p, k.c_cur, k, bad);                        // x + (1 v) dt = x + v dt, the same bits as x + dt v
    p = p + (V)((k.d_cur * (-E)) * k.dt);                        // v + (1 (-E)) dt = v + dt (-E)
  } else {
    p = p + (V)((k.d_cur * (-E)) * k.dt);                        // integration.py:32
    if (STAGE != ST_SE) {                                        // (VK, VM)
      q = xw;                                                    // pic.py:139 (+ util.py:51): the step ends here
      ke += (double)p * (double)p;
    }
    if (STAGE == ST_VM) p = p + (V)((k.d_cur * (-E)) * k.dt);    // the next step's first half-kick: same field, second addition
    if (STAGE != ST_VK) q = drift<P>(q, p, k.c_cur, k, bad);     // integration.py:42
  }
  if (STAGE != ST_VK) {
    locate<P, SHAPE, kFold>(q, k, xw, j, w, frac, bad);
    deposit<A, P, SHAPE>(acc, j, w, frac, k.magic);
    if (STAGE != ST_VM) {                                        // (VM stores the drifted q, as sweep C does: the next sweep wraps it)
      q = xw;
      ke += (double)p * (double)p;
    }
  }
  xq = q;
  vp = p;
}

// Total of one mesh node over the R LDS replicas of a workgroup, periodic ghost slots folded in, as an integer
// in units of 2^-fg (the unit of the global accumulators).  WIDE (CIC): slot Ng + 1 holds deposits too, those of node 1 made at
// the unfolded index Ng (kFoldIndex: the sweeps; the resident kernel folds the index and leaves the slot alone).
template <typename A, int SHAPE, bool WIDE = false>
__device__ __forceinline__ acc_t mesh_node_sum(const A* __restrict__ acc_all, int R, int stride, int Ng, int fg, int c) {
  constexpr int OFF = (SHAPE == PIC_TSC) ? 1 : 0;
  if constexpr (std::is_same<A, fix_t>::value) {
    const unsigned long long* a = reinterpret_cast<const unsigned long long*>(acc_all);
    const int cm = c == 0 ? Ng - 1 : c - 1;
    unsigned long long own = 0ull, left = 0ull;
    for (int r = 0; r < R; ++r) {
      own += a[(size_t)r * stride + c];
      left += a[(size_t)r * stride + cm];
    }
    const long long mask = (1ll << FX_LOW) - 1;
    const long long q = ((long long)(own >> FX_LOW) << FX_FRAC) - ((long long)own & mask) + ((long long)left & mask);
    return q << (fg - FX_FRAC);                                   // 2^-24 units -> 2^-fg units
  } else {
    A s = A(0);
    for (int r = 0; r < R; ++r) {
      const A* ar = acc_all + (size_t)r * stride;
      A t = ar[c + OFF];
      if (SHAPE == PIC_CIC) {
        if (c == 0) t += ar[Ng];
        if (WIDE && c == 1) t += ar[Ng + 1];
      } else {
        if (c == 0) t += ar[Ng + 1];
        if (c == Ng - 1) t += ar[0];
      }
      s += t;
    }
    if constexpr (std::is_same<A, acc_t>::value) return s;
    else return __double2ll_rn(ldexp((double)s, fg));
  }
}

// Add a workgroup's LDS mesh to the environment's global accumulator row with 64-bit integer atomics (executed
// at the memory side, order-independent; 16.8 MB per sweep at config 2, hidden under the streaming of the other
// resident workgroups: profiles/experiments_r2.md).
template <typename A, int SHAPE>
__device__ __forceinline__ void flush_mesh(const A* __restrict__ acc_all, int R, int stride, int Ng, int fg,
                                           acc_t* __restrict__ row) {
  unsigned long long* out = reinterpret_cast<unsigned long long*>(row);
  for (int c = threadIdx.x; c < Ng; c += BLOCK) {
    const acc_t q = mesh_node_sum<A, SHAPE, !kFoldIndex<A, SHAPE>>(acc_all, R, stride, Ng, fg, c);
    if (q) atomicAdd(out + c, (unsigned long long)q);
  }
}

// what a sweep reads its field from, where its deposits go, which retired accumulator rows it clears
struct SweepIO {
  // accumulator rows are [S][env][Ng] (S sub-rows, SweepArgs::S; pic_device.h: acc_row_sum)
  const acc_t* acc_in;     // deposit the field of this sweep's gather is solved from (gather stages)
  Control ctl;             // external field of the force evaluation: on the mesh or as actuator coefficients (environment 0's pointers)
  // The actuator's field is built ONCE per environment and step where the schedule allows it, not in every workgroup of every
  // sweep: ext_out [env][Ng] (or null) receives, from workgroup 0 of every environment, the field this sweep built from ctl.act
  // (sweep B of a call's first step: it cannot wait for anyone) or -- with ctl.ext and next_act -- the field of the NEXT step's
  // coefficients (sweep D inside a rollout).  The sweeps that follow read it as a mesh field (host_schedule.h: CTL_SHARED).
  double* ext_out;
  const double* next_act;  // [env][2M] coefficients of the next step (environment 0), or null
  acc_t* acc_out;          // receives this sweep's deposit (zero on entry; null in sweep D2, which makes none)
  acc_t* acc_out2;         // receives the next step's q1 deposit (D, D2, REFRESH) / the previous step's final positions (B2)
  acc_t* zero0;            // accumulators no kernel reads any more: cleared for a later sweep
  acc_t* zero1;
  double* ke_part;         // [env][nblk] sum of p^2 per workgroup (dual stages)
  unsigned long long* bad; // [1] count of non-finite / unrepresentable positions
  // Sweep C inside a multi-step pic_step call: the post-step refresh of the PREVIOUS step (pic.py:145-146) -- nothing this
  // step reads -- is done by one extra workgroup per environment (blockIdx.x == nblk) instead of a launch of its own, from the
  // deposit this step's sweep B2 made of the positions it read (rounds 2-3: sweep D deposited them and sweep B carried the solve).
  // post.acc == null: no such workgroup.
  SolveIO post;
  double* e2;              // [env][Ng + 2] field tile of a sweep that stores no particles (C_RO, B2_RO, D2_RO); the next launch re-derives
                           // that sweep's output from it (D_RC / D2_RC, C_RB, B2_RD)
};

constexpr size_t kSweepInlineOffset = 2 * sizeof(void*) + sizeof(SweepIO) + sizeof(SweepArgs);   // sweep_kernel(x, v, io, a, act_inline)
static_assert(sizeof(SweepIO) % 8 == 0 && sizeof(SweepArgs) % 8 == 0, "arguments lie back to back");

template <typename P, typename A, int SHAPE, int STAGE>
__global__ __launch_bounds__(BLOCK) void sweep_kernel(typename P::X* __restrict__ x, typename P::V* __restrict__ v,
                                                      SweepIO io, SweepArgs a, InlineDoubles act_inline) {
  constexpr int OFF = (SHAPE == PIC_TSC) ? 1 : 0;
  constexpr int VEC = P::VEC;
  using T = typename P::W;
  using XV = typename P::XV;
  using VV = typename P::VV;
  constexpr StageTraits kT = stage_traits(STAGE);
  constexpr bool kTileOut = leaves_tile(kT);                                   // stores no particles, but its field tile
  constexpr bool kTileIn = reads_tile(kT);                                     // re-derives the sweep before it from that tile
  constexpr bool kScheme = kT.arith == AR_SCHEME;                              // push_scheme's stages
  constexpr bool kGather = gathers(kT);
  constexpr bool kStore = kT.stores;
  constexpr bool kStoreV = kStore && kGather;                                  // (REFRESH stores its wrapped x alone)
  constexpr bool kAhead = !kStore;                                             // a loop without stores requests its tiles one ahead
  // ... and its whole tiles in the wave-uniform loop below, but for B2_RO on fixed-point positions: four particles per lane through
  // two deposits on two pairs of tile registers take 66-76 VGPRs there, 54-60 in the per-lane loop alone
  constexpr bool kUniform = kAhead && !(P::kFixed && STAGE == ST_B2_RO);
  constexpr bool kReadV = reads_v(kT);
  constexpr bool kDual = kT.second != M2_NONE;                                 // deposits into the second LDS mesh as well (-> acc_out2)

  // LDS: [R meshes: acc][R meshes: acc2 (dual stages)][field tile Es][the re-derived sweep's field tile Es2 (kTileIn)]; the mesh region is the scratch of the
  // prologue solve first
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int Ng = a.Ng;
  const int stride = Ng + 2;
  A* acc_all = reinterpret_cast<A*>(smem_raw);
  A* acc2_all = acc_all + (size_t)a.R * stride;
  T* Es = reinterpret_cast<T*>(smem_raw + (size_t)2 * a.R * stride * sizeof(A));
  T* Es2 = Es + stride;
  __shared__ double red[2 * WAVES];
  __shared__ double slot[2];       // mean of the prologue solve's gradient (16 B: keeps the dynamic LDS base aligned)
  static_assert(sizeof(red) + sizeof(slot) == kSweepStaticLds, "pic_create adds the static LDS to the dynamic part it sizes");
  PIC_STAMP(0);

  if (carries_solve(kT) && blockIdx.x == (unsigned)a.nblk) {      // the extra workgroup of its environment (host: only with io.post.acc)
    // its arguments are read from the kernel-argument segment here, by this workgroup alone: held in scalar registers from the
    // kernel's entry on they cost every other workgroup of the sweep a wave of occupancy (pic_device.h: kernarg_at)
    SolveIO post = kernarg_at<SolveIO>(2 * sizeof(void*) + offsetof(SweepIO, post));   // x, v, io, a
    post.out.fb = Feedback{};                                  // (the feedback law's solves are launches of their own)
    solve_environment(post, blockIdx.y, Ng, a.nblk, a.fg, a.S, a.sub, a.scale, a.n0, a.dx, a.N_over_L, smem_raw, red, slot);
    return;
  }

  const int tid = threadIdx.x;
  // Consecutive sweeps walk memory in opposite directions: what the previous sweep wrote last (still
  // in the 256 MB Infinity Cache) is what this one reads first.
  const int env = a.reverse ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;
  const int blk = a.reverse ? a.nblk - 1 - (int)blockIdx.x : (int)blockIdx.x;

  typename P::X* xe = x + (size_t)env * a.ld;
  typename P::V* ve = v + (size_t)env * a.ld;
  const long long step = (long long)BLOCK * VEC;
  // A workgroup owns one contiguous run of `chunk` particles of its environment; a lane streams 16 B of x and
  // 16 B of v per iteration and updates them in place.  The first tile is requested before the prologue, so that
  // its latency runs under the field solve -- but behind the accumulator row the solve starts from.
  const long long begin = (long long)blk * a.chunk;
  long long end = begin + a.chunk;
  if (end > a.N) end = a.N;
  long long i = begin + (long long)tid * VEC;
  AccRequest first_node{};            // the accumulator row goes first: the prologue waits for it, the tile is not needed before the push
  if (kGather) first_node = acc_row_request(io.acc_in + (size_t)env * Ng, tid < Ng ? tid : Ng - 1, a.S, a.sub);   // (no branch: see acc_row_request)
  // (unconditional, from a clamped address where the lane has no first tile: the row is padded to 64 elements.  A load under
  // a branch costs the exact vmcnt bookkeeping, and the prologue would wait for the tile as well as for the row)
  const long long i_first = (i + VEC <= end) ? i : 0;
  XV xv = stream_load(reinterpret_cast<const XV*>(xe + i_first));
  VV vv = {};
  if (kReadV) vv = stream_load(reinterpret_cast<const VV*>(ve + i_first));
  PIC_STAMP(2);

  // LDS of the prologue: b / G in the SECOND mesh's place; the first mesh is cleared while the accumulator row is on its way
  // (with an actuator its field takes that place first).  A sweep that deposits one mesh and has no actuator field to build
  // goes from the field tile's barrier straight to its particles.
  bool clear_first = true;
  if (kGather) {
    Control ctl = io.ctl;
    if (ctl.ext) ctl.ext += (size_t)env * Ng;
    // (a.act_inline: the call's actuator coefficients [num_envs][2M] are the kernel's last argument -- read through a pointer
    // into the argument segment -- instead of an array a copy or a launch in front of the step would have had to fill)
    if (a.act_inline) ctl.act = kernarg_ptr<double>(kSweepInlineOffset);
    if (ctl.act) ctl.act += (size_t)env * 2 * ctl.M;
    else {
      for (int c = tid; c < a.R * stride; c += BLOCK) acc_all[c] = A{};
      clear_first = false;
    }
    prologue_field<T, OFF>(io.acc_in + (size_t)env * Ng, first_node, a.S, a.sub, ctl,
                           (io.ext_out && blk == 0) ? io.ext_out + (size_t)env * Ng : nullptr, Ng, ldexp(1.0, -a.fg), a.scale, a.n0, a.dx,
                           reinterpret_cast<double*>(acc2_all), reinterpret_cast<double*>(smem_raw), slot, Es);
  }
  // (never both, stage_traits_hold: there is one tile buffer, and the sweep that reads a tile is the launch right behind its writer)
  if (kTileOut && blk == 0)             // the field tile of this force evaluation, for the sweep that re-derives it
    for (int c = tid; c < stride; c += BLOCK) io.e2[(size_t)env * stride + c] = (double)Es[c];
  if (kTileIn)                           // (the barrier behind the mesh clearing below covers these LDS writes)
    for (int c = tid; c < stride; c += BLOCK) Es2[c] = (T)io.e2[(size_t)env * stride + c];
  if (kT.arith == AR_D && io.next_act && io.ext_out && blk == 0) {   // (inside a rollout: one workgroup per environment)
    const Control ctl = io.ctl;
    for (int j = tid; j < Ng; j += BLOCK)
      io.ext_out[(size_t)env * Ng + j] = actuator_field(ctl.basis, ctl.basis + (size_t)Ng * ctl.M, io.next_act + (size_t)env * 2 * ctl.M, j, ctl.M);
  }
  if (clear_first) for (int c = tid; c < a.R * stride; c += BLOCK) acc_all[c] = A{};
  if (kDual) for (int c = tid; c < a.R * stride; c += BLOCK) acc2_all[c] = A{};
  if (blk < a.S) {      // workgroup s of an environment clears sub-row s of the retired accumulator rows
    const size_t z = (size_t)blk * a.sub + (size_t)env * Ng;
    if (io.zero0) for (int c = tid; c < Ng; c += BLOCK) io.zero0[z + c] = 0;
    if (io.zero1) for (int c = tid; c < Ng; c += BLOCK) io.zero1[z + c] = 0;
  }
  if (clear_first || kDual || kTileIn) __syncthreads();
  PIC_STAMP(6);

  const int rep = (tid >> 6) & (a.R - 1);
  A* acc = acc_all + (size_t)rep * stride;
  A* acc2 = acc2_all + (size_t)rep * stride;
  const Consts<P> k(a);

  double ke = 0.0;
  unsigned bad = 0u;
  [[maybe_unused]] int tile = 0;
  const StreamOut xout(xe + begin), vout(ve + begin);
  if constexpr (kUniform) {
    // The whole tiles of a chunk, nfull of them, are the same for every lane of the workgroup: the tiles whose SUCCESSOR is a whole
    // tile too run here, on a trip count and a tile base that are wave-uniform -- no per-lane index, end test or clamped address,
    // and the next tile's loads leave unconditionally from a pointer that advances by a constant.  Two tiles per trip, on two
    // pairs of registers that take turns, so that no tile is copied from "next" to "current".  The last whole tile, the partial
    // one and the lane tail stay with the per-lane loop below, which alone may meet a tile that some lanes do not have (and
    // alone prefetches from a clamped address: nothing is read here that is not pushed).
    const int nfull = (int)((end - begin) / step);
    if (nfull >= 2) {
      // (addresses as a wave-uniform base, advanced in scalar registers, plus the lane's constant 32-bit offset: the form a
      // load takes without any address arithmetic on the VALU.  The empty asm pins the base to scalar registers at each load;
      // left to itself the optimiser re-associates base and offset into per-lane 64-bit pointers again)
      // (global address space, spelled out: behind the asm the compiler cannot infer it and would emit flat loads)
      using GlobalBytes = const __attribute__((address_space(1))) char*;
      GlobalBytes xp = (GlobalBytes) reinterpret_cast<const char*>(xe + begin);
      GlobalBytes vp = (GlobalBytes) reinterpret_cast<const char*>(ve + begin);
      unsigned lane_off = (unsigned)tid * (unsigned)sizeof(XV);
      asm("" : "+v"(lane_off));
      constexpr size_t kTileBytes = (size_t)BLOCK * sizeof(XV);
      static_assert(sizeof(XV) == sizeof(VV), "one lane offset serves both streams");
      auto tile_x = [&](GlobalBytes base) __attribute__((always_inline)) {
        asm("" : "+s"(base));
        return *reinterpret_cast<const __attribute__((address_space(1))) XV*>(base + lane_off);
      };
      auto tile_v = [&](GlobalBytes base) __attribute__((always_inline)) {
        asm("" : "+s"(base));
        return *reinterpret_cast<const __attribute__((address_space(1))) VV*>(base + lane_off);
      };
      auto push_tile = [&](XV& xt, VV& vt) __attribute__((always_inline)) {
        typename P::X* xs = reinterpret_cast<typename P::X*>(&xt);
        typename P::V* vs = reinterpret_cast<typename P::V*>(&vt);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          typename P::V pv = kReadV ? vs[c] : typename P::V(0);
          push_one<P, A, SHAPE, STAGE>(xs[c], pv, Es, Es2, acc, acc2, k, ke, bad);
        }
      };
      XV xw;
      VV vw = {};
      int left = nfull - 1;                                  // tiles with a whole successor
      for (; left >= 2; left -= 2) {
        PIC_STAMP_LOADS(8 + 2 * tile);
        xw = tile_x(xp + kTileBytes);
        if (kReadV) vw = tile_v(vp + kTileBytes);
        push_tile(xv, vv);
        PIC_STAMP(9 + 2 * tile);
        ++tile;
        xp += 2 * kTileBytes;
        vp += 2 * kTileBytes;
        PIC_STAMP_LOADS(8 + 2 * tile);
        xv = tile_x(xp);
        if (kReadV) vv = tile_v(vp);
        push_tile(xw, vw);
        PIC_STAMP(9 + 2 * tile);
        ++tile;
      }
      if (left) {                                            // an odd one: once per workgroup, with the copy
        PIC_STAMP_LOADS(8 + 2 * tile);
        xw = tile_x(xp + kTileBytes);
        if (kReadV) vw = tile_v(vp + kTileBytes);
        push_tile(xv, vv);
        PIC_STAMP(9 + 2 * tile);
        ++tile;
        xv = xw;
        vv = vw;
      }
      i += (long long)(nfull - 1) * step;
    }
  }
  while (i + VEC <= end) {
    PIC_STAMP_LOADS(8 + 2 * tile);
    // A sweep that stores nothing requests its NEXT tile here, into a second pair of registers, before it pushes this one: the
    // loads run under the tile's arithmetic inside the wave, not only under that of the other waves.  Unconditional, from a
    // clamped address behind the last tile (as the first tile's: one line for the whole wave).  With no store in the loop the
    // compiler counts the loads exactly: the next tile's stay in flight under this tile's arithmetic.
    [[maybe_unused]] XV xv_next;
    [[maybe_unused]] VV vv_next = {};
    if constexpr (kAhead) {
      const long long i_next = (i + step + VEC <= end) ? i + step : 0;
      xv_next = stream_load(reinterpret_cast<const XV*>(xe + i_next));
      if (kReadV) vv_next = stream_load(reinterpret_cast<const VV*>(ve + i_next));
    }
    typename P::X* xs = reinterpret_cast<typename P::X*>(&xv);
    typename P::V* vs = reinterpret_cast<typename P::V*>(&vv);
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      typename P::V pv = kReadV ? vs[c] : typename P::V(0);
      if constexpr (kScheme) push_scheme<P, A, SHAPE, STAGE>(xs[c], pv, Es, acc, k, ke, bad);
      else push_one<P, A, SHAPE, STAGE>(xs[c], pv, Es, Es2, acc, acc2, k, ke, bad);
      if (kReadV) vs[c] = pv;
    }
    if (kStore) {
      xout.store((int)((i - begin) * (long long)sizeof(typename P::X)), xv);
      if (kStoreV) vout.store((int)((i - begin) * (long long)sizeof(typename P::V)), vv);
    }
    PIC_STAMP(9 + 2 * tile);
    ++tile;
    i += step;
    if constexpr (kAhead) {
      xv = xv_next;
      vv = vv_next;
    } else if (i + VEC <= end) {
      xv = stream_load(reinterpret_cast<const XV*>(xe + i));
      if (kReadV) vv = stream_load(reinterpret_cast<const VV*>(ve + i));
    }
  }
  for (long long c = i; c < end; ++c) {       // ragged tail (fewer than VEC particles left for this lane)
    typename P::X xq = xe[c];
    typename P::V pv = kReadV ? ve[c] : typename P::V(0);
    if constexpr (kScheme) push_scheme<P, A, SHAPE, STAGE>(xq, pv, Es, acc, k, ke, bad);
    else push_one<P, A, SHAPE, STAGE>(xq, pv, Es, Es2, acc, acc2, k, ke, bad);
    if (kStore) {
      xe[c] = xq;
      if (kStoreV) ve[c] = pv;
    }
  }
  __syncthreads();
  PIC_STAMP(24);

  const size_t sub_row = (size_t)(blk % a.S) * a.sub + (size_t)env * Ng;
  if (kT.first) flush_mesh<A, SHAPE>(acc_all, a.R, stride, Ng, a.fg, io.acc_out + sub_row);
  if (kDual) flush_mesh<A, SHAPE>(acc2_all, a.R, stride, Ng, a.fg, io.acc_out2 + sub_row);
  PIC_STAMP(25);

  if (ends_step(kT)) {                                   // sum of p^2 per workgroup
    double w = wave_sum(ke);
    if ((tid & 63) == 0) red[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int c = 0; c < WAVES; ++c) s += red[c];
      io.ke_part[(size_t)env * a.nblk + blk] = s;
    }
  }
  if (bad) atomicAdd(io.bad, (unsigned long long)bad);
  PIC_STAMP_LOADS(26);
}

}  // namespace
