// picstep.hip -- MI355X (gfx950 / CDNA4) 1-D electrostatic PIC stepper behind the C ABI of
// include/picstep.h.  Written for wave64, LDS-resident per-block mesh tiles and coalesced SoA
// particle streams; there is no other backend and no CPU fallback.
//
// One environment step = PIC.update_state of the reference (src/env/pic.py:131-146), i.e. the
// Yoshida-4 composition of src/env/integration.py:60-75 restated as kick/drift sub-stages:
//
//   [sweep A: q1 = x + (c1 v) dt ; deposit(q1)]   -- normally NOT run: the previous sweep D (or the
//                                                    reset sweep) has already deposited this q1
//   sweep B : E = field(deposit of q1) + E_ext ; p1 = v + (d1 (-E(q1))) dt ; q2 = q1 + (c2 p1) dt ; deposit(q2)
//   sweep C : E = field(deposit of q2) + E_ext ; p2 = p1 + (d2 (-E(q2))) dt ; q3 = q2 + (c3 p2) dt ; deposit(q3)
//   sweep D : E = field(deposit of q3) + E_ext ; p3 = p2 + (d3 (-E(q3))) dt ; q4 = q3 + (c4 p3) dt ;
//             x' = mod(q4, L) ; deposit(x') ; KE partials ; store x', p3 ;
//             deposit(next q1 = x' + (c1 p3) dt) into a second mesh
//   solve   : n, E_mesh (no E_ext), phi, KE, PE, PE_reward        (pic.py:145-146, util.py:119-147)
//
// 4 launches and 3 read+write passes over the particles per step (96 B per particle-step in fp64).  Inside a multi-step
// pic_step call every step but the last ends with sweep D2 = D without deposit(x'); the next step's sweep B2 = B + deposit of the
// positions it reads (that x') makes it instead -- D is the one sweep bound by VALU issue, B is bound by memory -- and the post-step
// solve of the step rides with that step's sweep C (one extra workgroup per environment): 3 launches per step there.  Every
// sweep workgroup solves the field it gathers from in its own prologue (pic_sweep.h: prologue_field), from
// the accumulator row the previous sweep filled.
//
// Arithmetic inside a sub-stage keeps the reference's operand order and is compiled with
// -ffp-contract=off so that fp64 results track NumPy to rounding (tests/ hold the bounds).
//
// Deposit: every workgroup owns an LDS copy of its environment's mesh (two in sweep D: final positions and the next step's
// first drift) and accumulates with integer LDS atomics (weights as 2^-fg fixed point, or one packed word per particle for
// single-precision CIC; pic_device.h), then adds its partial mesh to the environment's row [env][Ng] of a
// global 64-bit fixed-point accumulator with memory-side integer atomics.  Integer sums are order-independent:
// a step is bitwise reproducible and does not depend on the launch geometry.  Accumulator rows rotate through a
// small ring; a row whose readers are done is cleared by a later sweep (no memset launches).
//
// Files: pic_limits.h (launch constants), pic_device.h (particle formats, per-particle helpers, scans), pic_sweep.h (push sweeps),
// pic_solve.h (field solve), pic_aux.h (kernels off the step path); host_plan.h (pic_create's argument checks and the launch plan:
// no HIP, pinned on a CPU by tests/test_plan_cpu.py), host_blocks.h (the layout of every carved device block: no HIP either, pinned by
// tests/test_blocks_cpu.py), host_place.h (the search for a placement of x and v); this file holds the
// handle, the launch schedule and the C ABI, but for the host side of the differentiable rollouts: host_diff.h, host_phase.h,
// host_tape.h, host_tangent.h, host_tangent_walk.h.  pic_copy.h, host_copy.h and host_copy_map.h: copies of whole environments (pic_copy_envs).
// pic_policy.h and host_policy.h: the MLP policy of pic_policy_eval and pic_step_policy.
// pic_pool.h and host_pool.h: the pooled particle features of pic_pool and pic_pool_vjp, as passes over a layer type;
// pic_pool_ln.h: the layer type of pic_pool_ln and pic_pool_ln_vjp (a LayerNorm inside the per-particle layer).
// pic_actor.h and host_actor.h: the DeepSets particle actor of pic_actor_eval and pic_step_actor (the pooled features and a head).
// host_head.h: what the calls of the two controllers share (its parameter count and shape check: no HIP, tests/test_head_cpu.py).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "picstep.h"

#include "host_plan.h"
#include "host_copy_map.h"
#include "host_blocks.h"
#include "host_schedule.h"

#include "pic_device.h"
#include "pic_sweep.h"
#include "pic_solve.h"
#include "pic_resident.h"
#include "pic_aux.h"
#include "pic_record.h"
#include "pic_adjoint.h"
#include "pic_tangent.h"
#include "pic_phase.h"
#include "pic_moments.h"
#include "pic_copy.h"
#include "pic_policy.h"
#include "pic_pool.h"
#include "pic_pool_ln.h"
#include "pic_actor.h"


// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
namespace {

typedef pic_placement PlacementStats;
struct PlacementState {
  size_t pbytes = 0;                  // size of x and of v (0: no search on this handle)
  int legs = 0;                       // legs run so far
  size_t frontier = 0;                // blocks the longest leg has walked over: a later leg takes no readings before that
  double best_n = 0.0, worst_n = 0.0; // normalised readings of the block kept and of the slowest pair seen (0: none yet)
  bool found = false;
  bool ptrs_exposed = false;          // pic_device_ptrs has handed out the addresses of x and v: v stays where it is
  bool x_cleared = false;
};

// The owner of one HIP resource (device block, pinned host block, event, stream): move-only, releases what it holds at most once
// (an empty owner releases nothing), and converts to the raw handle, so that launches and argument blocks take it as they did
// the pointer.
template <typename P, auto Release>
class Owner {
 public:
  Owner() = default;
  explicit Owner(P p) : p_(p) {}
  Owner(Owner&& o) noexcept : p_(o.release()) {}
  Owner& operator=(Owner&& o) noexcept { reset(o.release()); return *this; }
  ~Owner() { reset(); }
  void reset(P p = nullptr) {
    if (p_ && p_ != p) (void)Release(p_);
    p_ = p;
  }
  P release() { P p = p_; p_ = nullptr; return p; }
  P get() const { return p_; }
  operator P() const { return p_; }

 private:
  P p_ = nullptr;
};
template <typename T> using DeviceBuf = Owner<T*, hipFree>;
template <typename T> using PinnedBuf = Owner<T*, hipHostFree>;
using EventOwner = Owner<hipEvent_t, hipEventDestroy>;
using StreamOwner = Owner<hipStream_t, hipStreamDestroy>;

// b lets its block go, then holds `bytes` of new memory (or nothing: the allocation's error is returned)
template <typename T>
hipError_t alloc(DeviceBuf<T>& b, size_t bytes) {
  b.reset();
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess) b.reset(static_cast<T*>(p));
  return e;
}
template <typename T>
hipError_t alloc(PinnedBuf<T>& b, size_t bytes) {
  b.reset();
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  if (e == hipSuccess) b.reset(static_cast<T*>(p));
  return e;
}
// alloc, then the block zeroed on `stream`
template <typename T>
hipError_t alloc_zeroed(DeviceBuf<T>& b, size_t bytes, hipStream_t stream) {
  const hipError_t e = alloc(b, bytes);
  return e != hipSuccess ? e : hipMemsetAsync(b, 0, bytes, stream);
}
inline EventOwner make_event() {        // empty if hipEventCreate fails
  hipEvent_t e = nullptr;
  return EventOwner(hipEventCreate(&e) == hipSuccess ? e : nullptr);
}

// The rollout recorder of a handle (pic_record_*, pic_record.h).  Records live in two device arrays, one slot per record:
// doubles [cap][env][d_stride] (KE, PE, PE_reward, field_energy, entropy, kl, re [M], im [M]) and uint32 [cap][env][u_stride]
// (x_hist, v_hist, inside), the latter zeroed when recording starts; the step indices are known here.
struct Recorder {
  bool on = false;
  int stride = 1, M = 0, xb = 0, vb = 0, px = 0, pv = 0;
  double vmin = 0, vmax = 0, pdx = 0, pdv = 0;
  int64_t cap = 0;
  int64_t k = 0;                      // steps made since pic_record_start
  std::vector<int64_t> steps;         // step index of every record held
  long long d_stride = 0, u_stride = 0;
  DeviceBuf<double> d;
  DeviceBuf<unsigned> u;
  DeviceBuf<unsigned> phase;          // [env][px pv] counts of the record being made (zero between records)
  DeviceBuf<double> feq;              // [px pv] or null
  RecordPlan plan;                    // the particle pass's grid and LDS layout (host_blocks.h: record_plan)
};

// One carved device block of the tape and the bytes it counts in Tape::bytes; host_diff.h: tape_reserve is the one place that
// allocates, carves and counts one
struct TapeBlock {
  DeviceBuf<void> mem;
  size_t bytes = 0;
  explicit operator bool() const { return mem.get() != nullptr; }
};

// The tape of a differentiable rollout (pic_tape_*, pic_adjoint.h).  One device block holds the checkpoints
// (x, v every `every` steps, the first at pic_tape_start), every step's external field and all the backward's working memory,
// (a-bar included), so that pic_tape_backward allocates nothing: TapeViews (host_blocks.h) are the views into it.  Everything
// attached to a tape later is a member struct: its block, the views into it (its base, laid out in host_blocks.h) and its state.
// Every block counts in `bytes`.
struct Tape : TapeViews {
  bool on = false;
  int64_t max_steps = 0, every = 1, steps = 0, nck = 0;
  size_t bytes = 0;
  TapeBlock block;
  unsigned long long* counters = nullptr;   // cmax + env: [0] replay mismatches of the last backward or tangent, [1] replay positions out of range
  int64_t launches = 0;               // kernels the last backward or tangent enqueued
  int64_t budget = 0;                 // budget_bytes of pic_tape_start (0: none)
  // steps of the gain law (pic_step_feedback_gain): the block comes with the first such call, one gain per call
  struct Law : LawViews {
    TapeBlock block;
    std::vector<int> step;            // [max_steps] per step: the index of its gain in `gains`, or -1 (empty: no law step yet)
    std::vector<DeviceBuf<double>> gains;   // per call: [env][2M][2M]
  } law;
  // the reverse walk (pic_tape_walk_*); pic_tape_backward[_feedback] is a walk of its own.  Any append, start,
  // stop, backward, tangent, tangent walk or new walk abandons it.
  struct Walk {
    bool on = false;                  // a walk is in progress
    int64_t next = -1;                // the next step it reverses (-1: all walked)
    int mo = 0;                       // M_o: modes of the walk's mode cotangents
    DeviceBuf<double> stage;          // [2][env][N] + [env][2 M_o] host cotangents of a step on the device (allocated on demand)
    size_t stage_bytes = 0;
    DeviceBuf<double> E;              // [env][Ng] E-bar of a walk's mode cotangents on a tape without a law block (else law.E)
  } walk;
  // forward mode (pic_tape_tangent): the tangent state, meshes and unit words of k directions, allocated by the
  // first call with that many and grown for more
  struct Tan {
    TapeBlock block;
    int k = 0;
    TanArgs views{};                  // st, dF, acc, ke, umax (host_tangent.h: tangent_args fills in the rest)
  } tan;
  // the forward walk through closed loops (pic_tape_tangent_walk_*, pic_tape_tangent_feedback): its working rows
  // for cap_k directions and cap_mo observed modes, allocated by the first walk and grown for more.  It replays into the segment
  // buffer as the reverse walk does, so either abandons the other; any append, start, stop, backward or tangent abandons it too.
  struct TanWalk : TanWalkViews {
    TapeBlock block;
    int cap_k = 0, cap_mo = 0;
    bool on = false;                  // a forward walk is in progress
    int64_t next = 0;                 // the next step it advances
    int k = 0, mo = 0;                // its directions and observed modes
    bool dgain = false;               // it carries a gain tangent
    bool policy = false;              // it goes through the policy's steps
  } twalk;
  // the per-step smoothed KL (pic_tape_kl_*): the block comes with pic_tape_kl_start
  struct Kl : KlViews {
    TapeBlock block;
    bool on = false;                  // a KL is attached: advance cuts behind every step and writes its row of the trace
    pic_phase_spec spec{};            // the caller's spec with feq = the tape's copy (device memory)
    std::vector<char> flag;           // [max_steps] per step: cot holds a row for it
  } kl;
  // forward mode of that KL (pic_tape_tangent_kl): the block comes with the first call that asks for d_kl
  struct TanKl : TanKlViews {
    TapeBlock block;
  } tkl;
  // cotangents on the fluid moments of the tape's states (pic_tape_moments_cot): the block comes with the first
  // call that sets a row
  struct MomCot : MomCotViews {
    TapeBlock block;
    std::vector<char> flag;           // [max_steps + 1] per row: cot holds a cotangent there
  } mom_cot;
  // the moments of every taped step (pic_tape_moments_start); trace set: advance cuts behind every step and writes its row
  struct MomTrace : MomTraceViews {
    TapeBlock block;
  } mom_trace;
  // forward mode of the moments (pic_tape_tangent_moments): one block for kMaxTangents directions, with the first
  // call that asks for d_moments
  struct TanMom {
    TapeBlock block;
    MomJvpArgs views{};               // acc, umax (the rest is a step's)
  } tmom;
  // steps under an MLP policy (pic_tape_step_policy): the block comes with the first such call, and every call
  // keeps a copy of its parameters and obs_scale
  struct Policy : TapePolicyViews {
    TapeBlock block;
    pic_policy shape{};               // the shape every policy call of this tape has (params, obs_scale: unused)
    size_t P = 0;                     // doubles of one parameter vector
    struct Copy { DeviceBuf<double> params; const double* scale; double action_scale; size_t bytes; };
    std::vector<Copy> calls;          // per call: params [P] or [env][P], then obs_scale [2 Mo] behind them (scale: null without)
    std::vector<int> step;            // [max_steps] per step: the index of its call in `calls`, or -1 (empty: no policy step yet)
    bool first = true;                // the reverse pass in progress has met no policy step yet: the next one starts gE's sums
    bool cot_obs = false, cot_act = false;   // cobs / cact hold a backward's cotangents
    bool valid = false;               // gE holds the sums of a finished reverse pass over the steps taped so far
  } policy;
  // forward mode through the policy's steps (pic_tape_tangent_policy): the working rows of cap_k directions next
  // to the walk's, allocated by the first call and grown for more
  struct TanPolicy : TanPolViews {
    TapeBlock block;
    int cap_k = 0;
    bool dparams = false;             // the walk in progress carries a parameter tangent
  } tpol;
};

}  // namespace

struct __attribute__((visibility("hidden"))) pic_handle : LaunchPlan {      // the plan: pic_create, once
  pic_config cfg{};
  int scheme = PIC_YOSHIDA4;          // time integrator of the steps (pic_set_integrator)
  hipStream_t stream = nullptr;       // the stream every call works on (own_stream, or the caller's)
  StreamOwner own_stream;             // created by pic_create (declared ahead of the buffers: destroyed after them)
  bool readonly_c = false;            // whole steps run sweeps C_RO and D_RC / D2_RC (pic_set_readonly_c, or readonly_auto)
  bool alternate_stores = false;      // ... and every second inner step of a call stores once (pic_set_alternate_stores, or alternate_auto)
  PlacementStats place{};             // what the search for an (x, v) placement did, all legs together (pic_placement_stats)
  PlacementState place_state{};       // what a later leg of it needs to know (placement_leg, resume_placement)
  Recorder rec{};                     // pic_record_*: reductions recorded after every rec.stride-th step (advance, pic_step_stage)
  Tape tape{};                        // pic_tape_*: checkpoints and external fields of a differentiable rollout (advance)
  DeviceBuf<void> x;
  void* v = nullptr;              // v_block, or a view into x's block (!v_separate)
  DeviceBuf<void> v_block;        // v's own allocation (v_separate)
  DeviceBuf<void> scratch;        // [env][ld] positions of a probe (eval_field / compute_E)
  DeviceBuf<void> stage;          // [env][N] float staging: fixed-point positions <-> the caller's floats
  // accumulator ring: rows [env][Ng] of 64-bit fixed-point weight sums
  DeviceBuf<acc_t> ring;
  Schedule sched;                 // which rows are clean, retired or hold a cached deposit, and the rest of what the streaming
                                  // schedule remembers between two calls (host_schedule.h)
  hipError_t ring_error = hipSuccess;   // a clearing memset of ring_take_clean that failed (reported by launch_status)
  acc_t* probe_acc = nullptr;     // view: ring's accumulator row of the probes (their own: a probe never touches step state)
  DeviceBuf<double> probe_ext;    // device copy of a probe's host E_ext
  DeviceBuf<double> ke_part;      // [env][nblk]
  DeviceBuf<double> n;
  DeviceBuf<double> E_mesh;
  DeviceBuf<double> phi;
  DeviceBuf<double> ext;          // device copy of a host E_ext / the actuator's field of a step, built once per environment (EXT_THIS)
  DeviceBuf<double> ext2;         // ... of the step after it (a rollout alternates between the two)
  DeviceBuf<double> e2;           // [env][Ng + 2] sweep C_RO's field tile, read by sweep D_RC / D2_RC
  DeviceBuf<double> basis;        // [2][Ng][M] actuator tables (cos, sin)
  DeviceBuf<double> act;          // [env][2M] actions: device copy of a host action / the feedback law's current action
  DeviceBuf<double> modes;        // [2][env][M] Fourier modes (re, im)
  int act_modes = 0;
  int modes_cap = 0;
  DeviceBuf<double> tw;           // [2][tw_rows][Ng] twiddles of modes 1..tw_rows (pic_aux.h: twiddle_kernel)
  int tw_rows = 0;
  DeviceBuf<void> traj;           // device copy of a host trajectory of actions or fields (pic_step_*_traj), grown on demand
  size_t traj_bytes = 0;
  DeviceBuf<unsigned long long> res_q1;   // resident schedule: [env][R (Ng + 2)] LDS mesh of the next step's q1 deposit, launch to launch
  bool res_q1_valid = false;
  DeviceBuf<void> res_carry;              // ... and the cell and weights of every particle's q1 (pic_resident.h: ResidentEdge), or null
  bool res_carry_valid = false;
  DeviceBuf<double> gain;         // [env][2M][2M] device copy of a host gain (pic_step_feedback_gain)
  DeviceBuf<double> fb_modes;     // [env][2 kMaxFeedbackModes] the gain law's m, step by step
  DeviceBuf<void> pol;            // the block of a policy call (host_policy.h: policy_parts), grown on demand
  size_t pol_bytes = 0;
  DeviceBuf<double> aux_n;        // probe outputs
  DeviceBuf<double> aux_E;
  DeviceBuf<double> aux_pe;
  PinnedBuf<double> h_probe_pe;   // pinned host: the energy of a probe, written by the solve itself (pic_eval_field of a small host state)
  bool probe_row_clean = false;   // the probes' accumulator row is zero (the solve of the last probe cleared it behind its read)
  DeviceBuf<double> aux_phi;
  DeviceBuf<double> KE;
  double* PE = nullptr;           // views into KE's block
  double* PEr = nullptr;
  PinnedBuf<double> h_scal;       // pinned host staging for KE | PE | PE_reward
  PinnedBuf<void> h_part;         // pinned host staging for x | v of states up to 64 MB (from pic_create on up to 4 MB, else on first use)
  bool h_part_refused = false;    // ... could not be had: do not ask again
  PinnedBuf<double> h_fields;     // pinned host staging for n | E_mesh | phi (meshes up to 256 KB each in total), or null
  DeviceBuf<void> mom_block;      // pic_moments, allocated by its first call
  MomViews mom;                   // views into it (host_blocks.h: moments_parts)
  DeviceBuf<void> pool_block;     // pic_pool, pic_pool_vjp: grows to what a call needs (host_blocks.h: pool_parts)
  size_t pool_cap = 0;            // its bytes
  size_t pool_zero = 0;           // ... of which the leading ones (max words, integer sums) are zero between calls
  DeviceBuf<unsigned long long> bad;
  unsigned long long* probe_bad = nullptr;   // view: bad + 1, where the probes count their non-finite positions (never read: pic_bad_count
                                             // describes the state's particles, and a probe's positions are not among them)
  bool has_state = false;
  // pic_copy_envs, all allocated by its first call
  DeviceBuf<int> copy_map;                    // [env] device copy of a host map
  DeviceBuf<unsigned long long> copy_rejected;   // entries of device maps refused by the kernels since pic_create
  EventOwner copy_ev[2];                      // a copy between two streams: behind the source's work, behind the copy's read
  // profiling
  bool prof = false;
  std::vector<EventOwner> ev;     // pairs
  std::vector<int> ev_kind;
  double ms_sum[8]{};
  int64_t launches[8]{};
  std::string err;
};

namespace {

thread_local std::string g_create_error;

#define HIPCHK(h, call)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
      return PIC_EHIP;                                                                        \
    }                                                                                         \
  } while (0)

int fail(pic_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

// f(PosF64{}), f(PosF32{}) or f(PosU32{}): the handle's particle format, the one place that turns h->fmt into a type.  A body
// writes its pointer casts as typename P::X* / typename P::V* with P = decltype(p).
template <typename F>
void with_format(const pic_handle* h, F&& f) {
  if (h->fmt == FMT_F64) f(PosF64{});
  else if (h->fmt == FMT_F32) f(PosF32{});
  else f(PosU32{});
}


// ---- accumulator ring -------------------------------------------------------------------------
size_t row_elems(const pic_handle* h) { return (size_t)h->S * h->cfg.num_envs * h->cfg.Ng; }       // one accumulator row: [S][env][Ng]
acc_t* ring_row(pic_handle* h, int slot) { return h->ring + (size_t)slot * row_elems(h); }

// Ring::take's guard was needed: `slot` came from the retired rows and is cleared here, ahead of the launch that fills it.  The
// step schedule does not get here (tests/test_schedule_cpu.py: no order of calls to depth 4, and no long random one, needs it).
// (a failure must not pass silently as a dirty row: it is kept for the caller's next check, launch_status below)
void ring_clear_late(pic_handle* h, int slot) {
  const hipError_t e = hipMemsetAsync(ring_row(h, slot), 0, row_elems(h) * sizeof(acc_t), h->stream);
  if (e != hipSuccess && h->ring_error == hipSuccess) h->ring_error = e;
}

// a zeroed row for a deposit made outside the step schedule (pic_copy_envs)
int ring_take_clean(pic_handle* h) {
  bool unclean = false;
  const int s = h->sched.ring.take(&unclean);
  if (unclean) ring_clear_late(h, s);
  return s;
}

// what the launches enqueued since the last check have left behind: the runtime's sticky error, or a failed row clearing
hipError_t launch_status(pic_handle* h) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) { e = h->ring_error; }
  h->ring_error = hipSuccess;
  return e;
}

template <typename P, typename A, int SHAPE, int STAGE>
void launch_sweep_t(pic_handle* h, const SweepIO& io, void* x, void* v, const SweepArgs& a, const InlineDoubles& act) {
  constexpr StageTraits t = stage_traits(STAGE);
  dim3 grid(h->nblk + ((carries_solve(t) && io.post.acc) ? 1 : 0), h->cfg.num_envs);
  const size_t lds = reads_tile(t) ? h->sweep_lds_rc : h->sweep_lds;
  hipLaunchKernelGGL((sweep_kernel<P, A, SHAPE, STAGE>), grid, dim3(BLOCK), lds, h->stream,
                     static_cast<typename P::X*>(x), static_cast<typename P::V*>(v), io, a, act);
}

// the instantiation for `stage` among those for S... = every Stage, 0 .. kStages - 1 (the step schedule hands on no other)
template <typename P, typename A, int SHAPE, int... S>
void launch_sweep_s(pic_handle* h, const SweepIO& io, int stage, void* x, void* v, const SweepArgs& a, const InlineDoubles& act, std::integer_sequence<int, S...>) {
  ((stage == S ? launch_sweep_t<P, A, SHAPE, S>(h, io, x, v, a, act) : void()), ...);
}

template <typename P>
void launch_sweep_p(pic_handle* h, const SweepIO& io, int stage, void* x, void* v, const SweepArgs& a, const InlineDoubles& act) {
  const bool tsc = h->cfg.interpol == PIC_TSC;
  const std::make_integer_sequence<int, kStages> all{};
  if constexpr (std::is_same<P, PosF64>::value) {
    if (h->acc_kind == PIC_ACC_F64) {
      if (tsc) launch_sweep_s<P, double, PIC_TSC>(h, io, stage, x, v, a, act, all);
      else launch_sweep_s<P, double, PIC_CIC>(h, io, stage, x, v, a, act, all);
      return;
    }
  } else {
    if (h->acc_kind == PIC_ACC_PACKED) { launch_sweep_s<P, fix_t, PIC_CIC>(h, io, stage, x, v, a, act, all); return; }
  }
  if (tsc) launch_sweep_s<P, acc_t, PIC_TSC>(h, io, stage, x, v, a, act, all);
  else launch_sweep_s<P, acc_t, PIC_CIC>(h, io, stage, x, v, a, act, all);
}

// Per-launch HIP-event brackets on the handle's stream.  Events come from a pool that is only grown
// (never created inside a timed loop once warm) and recycled by prof_drain.
void prof_drain(pic_handle* h) {
  for (size_t i = 0; i < h->ev_kind.size(); ++i) {
    float ms = 0.f;
    hipEventSynchronize(h->ev[2 * i + 1]);
    if (hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]) == hipSuccess) {
      h->ms_sum[h->ev_kind[i]] += ms;
      h->launches[h->ev_kind[i]] += 1;
    }
  }
  h->ev_kind.clear();
}
void prof_reserve(pic_handle* h, size_t pairs) {
  while (h->ev.size() < 2 * pairs) {
    EventOwner e = make_event();
    if (!e) break;
    h->ev.push_back(std::move(e));
  }
}
void prof_begin(pic_handle* h, int kind) {
  if (!h->prof) return;
  if (h->ev_kind.size() >= 16384) prof_drain(h);
  const size_t i = h->ev_kind.size();
  prof_reserve(h, i + 1);
  hipEventRecord(h->ev[2 * i], h->stream);
  h->ev_kind.push_back(kind);
}
void prof_end(pic_handle* h) {
  if (!h->prof) return;
  hipEventRecord(h->ev[2 * (h->ev_kind.size() - 1) + 1], h->stream);
}

// The SweepArgs fields the push sweeps and the resident kernel share: geometry, fixed point, units.  The rest (the sweeps'
// partition, ring sub-rows and stage coefficients; the resident kernel's LDS replicas) is the caller's.
SweepArgs sweep_args(const pic_handle* h) {
  SweepArgs a{};
  a.N = h->cfg.N; a.ld = h->ld; a.Ng = h->cfg.Ng;
  a.fg = h->fg; a.magic = h->magic;
  a.L = h->cfg.L; a.dx = h->dx; a.dt = h->cfg.dt;
  a.rdx = h->fmt == FMT_F64 ? 1.0 / h->dx : (double)(1.0f / (float)h->dx);
  a.scale = h->scale; a.n0 = h->cfg.n0;
  a.to_units = 4294967296.0 / h->cfg.L;
  a.N_over_L = (double)h->cfg.N / h->cfg.L;
  return a;
}

// SolveArgs of a field solve that reads S sub-rows of its accumulator row
SolveArgs solve_args(const pic_handle* h, int S) {
  SolveArgs a{};
  a.N = h->cfg.N; a.Ng = h->cfg.Ng; a.nblk = h->nblk; a.fg = h->fg; a.L = h->cfg.L; a.dx = h->dx; a.n0 = h->cfg.n0;
  a.scale = h->scale; a.N_over_L = (double)h->cfg.N / h->cfg.L;
  a.S = S; a.sub = (long long)h->cfg.num_envs * h->cfg.Ng;
  return a;
}

template <typename P, typename A, int SHAPE, int PPT, int NW>
void launch_resident_t(pic_handle* h, const ResidentIO& io, const SweepArgs& a, const InlineDoubles& act) {
  if (h->scheme != PIC_YOSHIDA4) {      // the other integrators: a kernel of their own (pic_resident.h: resident_scheme_kernel)
    const dim3 grid(h->cfg.num_envs), block(NW * 64);
    auto* x = static_cast<typename P::X*>(h->x.get());
    auto* v = static_cast<typename P::V*>(h->v);
    if (h->scheme == PIC_SYMPLECTIC_EULER)
      hipLaunchKernelGGL((resident_scheme_kernel<P, A, SHAPE, PPT, NW, PIC_SYMPLECTIC_EULER>), grid, block, h->res_lds, h->stream, x, v, io, a, act);
    else if (h->scheme == PIC_VERLET)
      hipLaunchKernelGGL((resident_scheme_kernel<P, A, SHAPE, PPT, NW, PIC_VERLET>), grid, block, h->res_lds, h->stream, x, v, io, a, act);
    else
      hipLaunchKernelGGL((resident_scheme_kernel<P, A, SHAPE, PPT, NW, PIC_FORWARD_EULER>), grid, block, h->res_lds, h->stream, x, v, io, a, act);
    return;
  }
  // More environments than CUs and a slot count whose lean kernel fits 128 registers: two workgroups per CU beat
  // the 15 % the carried cell / weights save per workgroup (profiles/experiments_r2.md 5).
  // (carrying three TSC weights for 16 particles per lane would need more than 256 registers: that kernel is not even compiled,
  // pic_create sets res_lean for the shape)
  constexpr bool kCarryFits = !(SHAPE == PIC_TSC && PPT == 16);
  if constexpr (kCarryFits) {
    if (!h->res_lean) {
      hipLaunchKernelGGL((resident_kernel<P, A, SHAPE, PPT, NW, true>), dim3(h->cfg.num_envs), dim3(NW * 64), h->res_lds,
                         h->stream, static_cast<typename P::X*>(h->x.get()), static_cast<typename P::V*>(h->v), io, a, act);
      return;
    }
  }
  hipLaunchKernelGGL((resident_kernel<P, A, SHAPE, PPT, NW, false>), dim3(h->cfg.num_envs), dim3(NW * 64), h->res_lds,
                     h->stream, static_cast<typename P::X*>(h->x.get()), static_cast<typename P::V*>(h->v), io, a, act);
}

template <typename P, typename A, int SHAPE>
void launch_resident_s(pic_handle* h, const ResidentIO& io, const SweepArgs& a, const InlineDoubles& act) {
  switch (h->res_nw * 100 + h->res_ppt) {
    case 804: launch_resident_t<P, A, SHAPE, 4, 8>(h, io, a, act); break;
    case 808: launch_resident_t<P, A, SHAPE, 8, 8>(h, io, a, act); break;
    case 810: launch_resident_t<P, A, SHAPE, 10, 8>(h, io, a, act); break;
    default: launch_resident_t<P, A, SHAPE, 16, 8>(h, io, a, act); break;
  }
}

template <typename P>
void launch_resident_p(pic_handle* h, const ResidentIO& io, const SweepArgs& a, const InlineDoubles& act) {
  const bool tsc = h->cfg.interpol == PIC_TSC;
  if constexpr (!std::is_same<P, PosF64>::value) {
    if (h->acc_kind == PIC_ACC_PACKED) { launch_resident_s<P, fix_t, PIC_CIC>(h, io, a, act); return; }
  }
  if (tsc) launch_resident_s<P, acc_t, PIC_TSC>(h, io, a, act);
  else launch_resident_s<P, acc_t, PIC_CIC>(h, io, a, act);
}

// What drives the external field of the steps of one call (device pointers; see Control / Feedback in pic_device.h)
struct StepControl {
  Control ctl{};           // first step's field or action (environment 0)
  long long ext_step = 0;  // elements between consecutive steps' fields / actions (0: held for the whole call)
  long long act_step = 0;
  Feedback fb{};           // fb.M > 0: feedback law; fb.act_hist = device [nsteps][env][2M] record of the actions, or null
  // one held action of few coefficients, given on the host: inside the resident kernel's own argument block (no copy, no launch)
  int inline_n = 0;
  InlineDoubles inline_act{};

  // the control of the same call from its step s on (E environments): the per-step fields / actions and the feedback law's
  // per-step records (actions, the gain law's modes) moved on by s steps
  StepControl after(size_t s, int E) const {
    StepControl o = *this;
    if (o.ctl.ext) o.ctl.ext += s * ext_step;
    if (o.ctl.act) o.ctl.act += s * act_step;
    const size_t row = (size_t)E * 2 * fb.M;
    if (o.fb.act_hist) o.fb.act_hist += s * row;
    if (o.fb.modes_hist) o.fb.modes_hist += s * row;
    return o;
  }
};

// the entries of step s in a call's per-step records: energies hist [nsteps][3][env], particles snap [nsteps][2][env][N]
// (either may be null)
double* hist_at(const pic_handle* h, double* hist, size_t s) { return hist ? hist + s * 3 * h->cfg.num_envs : nullptr; }
void* snap_at(const pic_handle* h, void* snap, size_t s) {
  return snap ? static_cast<char*>(snap) + s * 2 * h->cfg.num_envs * (size_t)h->cfg.N * h->esz : nullptr;
}

// nsteps environment steps in one launch of the resident schedule; hist: device [nsteps][3][env] or null
void launch_resident(pic_handle* h, const StepControl& sc, int nsteps, double* hist, void* snap = nullptr) {
  SweepArgs a = sweep_args(h);
  a.R = h->res_R;
  ResidentIO io{};
  io.nsteps = nsteps; io.num_envs = h->cfg.num_envs;
  io.c1 = h->cs[0]; io.c2 = h->cs[1]; io.d1 = h->ds[1]; io.d2 = h->ds[2];
  io.c.ctl = sc.ctl; io.c.ext_step = sc.ext_step; io.c.act_step = sc.act_step; io.c.fb = sc.fb;
  io.o.n = h->n; io.o.E = h->E_mesh; io.o.phi = h->phi; io.o.KE = h->KE; io.o.PE = h->PE; io.o.PEr = h->PEr;
  io.o.hist = hist;
  io.e.snap = snap; io.e.bad = h->bad;
  // the LDS mesh with the next step's q1 deposit travels from launch to launch (pic_invalidate and every reload drop it)
  io.e.q1_in = h->res_q1_valid ? h->res_q1 : nullptr;
  io.e.q1_out = h->res_q1;
  io.e.carry_in = h->res_q1_valid && h->res_carry_valid ? h->res_carry : nullptr;
  io.e.carry_out = h->res_carry;
  io.mode = (sc.inline_n > 0 ? RM_ACT_INLINE : 0) | (sc.ctl.ext || sc.ctl.act || sc.fb.M > 0 ? RM_EXT : 0) | (sc.ext_step || sc.act_step ? RM_PER_STEP : 0) |
            (sc.fb.M > 0 ? RM_FEEDBACK : 0) | (snap ? RM_SNAP : 0) | (hist || sc.fb.M > 0 ? RM_RECORD : 0);
  prof_begin(h, 6);
  with_format(h, [&](auto p) { launch_resident_p<decltype(p)>(h, io, a, sc.inline_act); });
  prof_end(h);
}

void launch_solve(pic_handle* h, const SolveIO& io) {
  prof_begin(h, 4);
  hipLaunchKernelGGL(field_solve_kernel, dim3(h->cfg.num_envs), dim3(SBLOCK), h->solve_lds, h->stream, io,
                     solve_args(h, io.acc ? h->S : 1));
  prof_end(h);
}

// What the launches of one call need besides the schedule's descriptors.  It lives on the caller's stack for that call.
struct CallCtx {
  const StepControl* sc = nullptr;   // the call's control: its fields or actions, the feedback law, the inline action (null: none)
  double* hist = nullptr;            // device [nsteps][3][env] record of the energies, or null
  void* probe_x = nullptr;           // a field probe: the positions it deposits instead of the state's
};

// The one place that turns a Launch of the step schedule (host_schedule.h) into kernel arguments and a launch.
void run_launch(pic_handle* h, const CallCtx& cx, const Launch& d) {
  const int E = h->cfg.num_envs;
  if (d.stage == ST_SOLVE) {
    SolveIO o{};
    o.acc = ring_row(h, d.in);
    o.ke_part = h->ke_part; o.n = h->n; o.out.E = h->E_mesh; o.out.phi = h->phi;
    o.out.KE = h->KE; o.out.PE = h->PE; o.out.PEr = h->PEr;
    o.out.hist = hist_at(h, cx.hist, d.step); o.out.num_envs = E;
    if (d.feedback) {                // the action of step + 1 is the feedback law's on the field this solve leaves
      o.out.fb = cx.sc->after(d.step + 1, E).fb;
      o.out.fb.act_out = h->act;
    }
    launch_solve(h, o);
    return;
  }
  for (int k = 0; k < 2; ++k)
    if (d.unclean >> k & 1) ring_clear_late(h, d.fill[k]);
  auto row = [&](int slot) { return slot >= 0 ? ring_row(h, slot) : nullptr; };
  double* const field[2] = {h->ext.get(), h->ext2.get()};
  Control ctl{};
  if (d.ctl != CTL_NONE && cx.sc) {
    ctl = cx.sc->after(d.step, E).ctl;
    if (cx.sc->fb.M > 0) { ctl.act = h->act; ctl.ext = nullptr; }
    if (d.ctl == CTL_SHARED) { ctl.act = nullptr; ctl.ext = field[d.turn]; }
  }
  SweepArgs a = sweep_args(h);
  a.chunk = h->chunk; a.nblk = h->nblk; a.R = h->R;
  a.act_inline = (ctl.act && cx.sc->inline_n > 0) ? 1 : 0;      // the held action rides in the sweep's argument block
  a.reverse = d.reverse;
  a.S = h->S; a.sub = (long long)E * h->cfg.Ng;
  a.c_prev = d.c_prev; a.d_prev = d.d_prev; a.c_cur = d.c_cur; a.d_cur = d.d_cur; a.c_next = h->cs[0];
  SweepIO io{};
  io.acc_in = row(d.in);
  io.ctl = ctl;
  if (d.ext_out != EXT_NONE) io.ext_out = field[d.ext_out == EXT_THIS ? d.turn : d.turn ^ 1];
  if (d.hand_on) io.next_act = cx.sc->after(d.step + 1, E).ctl.act;
  io.acc_out = row(d.fill[0]);
  io.acc_out2 = row(d.fill[1]);
  io.zero0 = row(d.clear[0]);
  io.zero1 = row(d.clear[1]);
  io.ke_part = h->ke_part;
  io.bad = d.fill[0] == RING ? h->probe_bad : h->bad;
  io.e2 = h->e2;
  if (d.post >= 0) {               // sweep C also carries the previous step's post-step refresh (pic_sweep.h: SweepIO::post)
    io.post.acc = ring_row(h, d.post);
    io.post.ke_part = h->ke_part; io.post.n = h->n; io.post.out.E = h->E_mesh; io.post.out.phi = h->phi;
    io.post.out.KE = h->KE; io.post.out.PE = h->PE; io.post.out.PEr = h->PEr;
    io.post.out.hist = hist_at(h, cx.hist, d.post_step); io.post.out.num_envs = E;
  }
  void* x = cx.probe_x ? cx.probe_x : h->x.get();
  void* v = cx.probe_x ? cx.probe_x : h->v;
  static const InlineDoubles none{};
  const InlineDoubles& act = a.act_inline ? cx.sc->inline_act : none;
  // (the particle sweeps of the other integrators -- Verlet's opening sweep is a sweep C -- count in the eighth kind)
  prof_begin(h, (d.stage == ST_C && h->scheme != PIC_YOSHIDA4) ? 7 : profile_kind(stage_traits(d.stage)));
  with_format(h, [&](auto p) { launch_sweep_p<decltype(p)>(h, io, d.stage, x, v, a, act); });
  prof_end(h);
}

void drop_cached_deposits(pic_handle* h) {
  plan_drop(h->sched);
  h->res_q1_valid = false;
}

int refresh_fields(pic_handle* h) {
  h->res_q1_valid = false;
  plan_refresh(h->sched, h->scheme, [&](const Launch& d) { run_launch(h, CallCtx{}, d); });
  HIPCHK(h, launch_status(h));
  return PIC_OK;
}

dim3 aux_grid(pic_handle* h, int nenv, long long cap = 1024) {
  long long gx = (h->cfg.N + BLOCK - 1) / BLOCK;
  if (gx > cap) gx = cap;
  return dim3((unsigned)gx, nenv);
}

// A buffer of the handle (re)allocated with `bytes`: the stream is drained if there is an old block (queued work may still read
// it), the old block goes, the new one takes its place.  On failure b is empty.
template <typename T>
int regrow(pic_handle* h, DeviceBuf<T>& b, size_t bytes, const char* what) {
  if (b) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (alloc(b, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(h, PIC_ENOMEM, what);
  }
  return PIC_OK;
}

int ensure_stage(pic_handle* h) {
  if (h->stage) return PIC_OK;
  HIPCHK(h, alloc(h->stage, (size_t)h->cfg.num_envs * h->cfg.N * sizeof(float)));
  return PIC_OK;
}

// ---- staging between the caller's memory and the device ------------------------------------------------------------------------
// the kind of a copy to or from the caller's memory: `host_kind` for PIC_HOST, else device to device
inline hipMemcpyKind copy_kind(int mem_kind, hipMemcpyKind host_kind) {
  return mem_kind == PIC_HOST ? host_kind : hipMemcpyDeviceToDevice;
}

// rows of device memory from the caller's src in mem_kind's memory, or zeros for a null src
inline hipError_t device_fill(pic_handle* h, double* dst, const double* src, size_t bytes, int mem_kind) {
  return src ? hipMemcpyAsync(dst, src, bytes, copy_kind(mem_kind, hipMemcpyHostToDevice), h->stream) : hipMemsetAsync(dst, 0, bytes, h->stream);
}

// An input in device memory: src itself when it is device memory (or null), else its copy in `buf`, the caller's device memory
inline hipError_t device_input(pic_handle* h, const double* src, int kind, size_t bytes, double* buf, const double** out) {
  *out = src;
  if (!src || kind != PIC_HOST) return hipSuccess;
  *out = buf;
  return hipMemcpyAsync(buf, src, bytes, hipMemcpyHostToDevice, h->stream);
}

// Device memory for an output: dst itself when it is device memory (or null), else `buf`; device_result copies it to dst behind
// the kernels that wrote it
inline double* device_output(void* dst, int kind, double* buf) { return dst && kind == PIC_HOST ? buf : static_cast<double*>(dst); }
inline hipError_t device_result(pic_handle* h, void* dst, const double* dev, size_t bytes) {
  return dst && dev != dst ? hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
}

// the read-backs (dst <- src) of `bytes` each that the caller asked for (dst not null), enqueued in their order
struct Readback { void* dst; const void* src; };
inline hipError_t read_back(pic_handle* h, size_t bytes, std::initializer_list<Readback> copies) {
  for (const Readback& c : copies) {
    if (!c.dst) continue;
    if (hipError_t e = hipMemcpyAsync(c.dst, c.src, bytes, hipMemcpyDeviceToHost, h->stream)) return e;
  }
  return hipSuccess;
}

// KE | PE | PE_reward out of the pinned staging, behind the wait for the copy or kernel that filled it
void unpack_scalars(const pic_handle* h, double* KE, double* PE, double* PE_reward) {
  const size_t E = (size_t)h->cfg.num_envs, b = E * sizeof(double);
  if (KE) std::memcpy(KE, h->h_scal, b);
  if (PE) std::memcpy(PE, h->h_scal + E, b);
  if (PE_reward) std::memcpy(PE_reward, h->h_scal + 2 * E, b);
}

// copy a dense [env][N] caller array of velocities (or float positions) into a padded [env][ld] device array
int upload(pic_handle* h, void* dst_padded, const void* src, int mem_kind) {
  const size_t row = (size_t)h->cfg.N * h->esz;
  HIPCHK(h, hipMemcpy2DAsync(dst_padded, (size_t)h->ld * h->esz, src, row, row, h->cfg.num_envs,
                             copy_kind(mem_kind, hipMemcpyHostToDevice), h->stream));
  return PIC_OK;
}

// positions arrive as floats of the particle dtype; the fixed-point format converts them on the device
int upload_positions(pic_handle* h, void* dst_padded, const void* src, int mem_kind, unsigned long long* bad) {
  if (h->fmt != FMT_U32) return upload(h, dst_padded, src, mem_kind);
  const float* dsrc = static_cast<const float*>(src);
  if (mem_kind == PIC_HOST) {
    int rc = ensure_stage(h);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->stage, src, (size_t)h->cfg.num_envs * h->cfg.N * sizeof(float), hipMemcpyHostToDevice, h->stream));
    dsrc = static_cast<const float*>(h->stage.get());
  }
  hipLaunchKernelGGL((positions_in_kernel<PosU32, float>), aux_grid(h, h->cfg.num_envs), dim3(BLOCK), 0, h->stream, dsrc,
                     static_cast<unsigned*>(dst_padded), h->cfg.N, h->ld, h->cfg.L, bad);
  HIPCHK(h, hipGetLastError());
  return PIC_OK;
}

int download(pic_handle* h, void* dst, const void* src_padded, int mem_kind) {
  const size_t row = (size_t)h->cfg.N * h->esz;
  HIPCHK(h, hipMemcpy2DAsync(dst, row, src_padded, (size_t)h->ld * h->esz, row, h->cfg.num_envs,
                             copy_kind(mem_kind, hipMemcpyDeviceToHost), h->stream));
  return PIC_OK;
}

int download_positions(pic_handle* h, void* dst, const void* src_padded, int mem_kind) {
  if (h->fmt != FMT_U32) return download(h, dst, src_padded, mem_kind);
  float* ddst = static_cast<float*>(dst);
  if (mem_kind == PIC_HOST) {
    int rc = ensure_stage(h);
    if (rc) return rc;
    ddst = static_cast<float*>(h->stage.get());
  }
  hipLaunchKernelGGL((positions_out_kernel<PosU32, float>), aux_grid(h, h->cfg.num_envs), dim3(BLOCK), 0, h->stream,
                     static_cast<const unsigned*>(src_padded), ddst, h->cfg.N, h->ld, h->cfg.L);
  HIPCHK(h, hipGetLastError());
  if (mem_kind == PIC_HOST)
    HIPCHK(h, hipMemcpyAsync(dst, h->stage, (size_t)h->cfg.num_envs * h->cfg.N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  return PIC_OK;
}

// mesh [env][Ng] gathered at the positions x [env][ld] with the handle's shape function -> out, dense [env][N]
void launch_gather(pic_handle* h, const void* x, const double* mesh, void* out) {
  const dim3 grid = aux_grid(h, h->cfg.num_envs);
  with_format(h, [&](auto p) {
    using P = decltype(p);
    const size_t lds = ((size_t)h->cfg.Ng + 2) * sizeof(typename P::W);
    if (h->cfg.interpol == PIC_TSC)
      hipLaunchKernelGGL((gather_E_kernel<P, PIC_TSC>), grid, dim3(BLOCK), lds, h->stream, (const typename P::X*)x, mesh,
                         (typename P::W*)out, h->cfg.N, h->ld, h->cfg.Ng, h->cfg.L, h->dx);
    else
      hipLaunchKernelGGL((gather_E_kernel<P, PIC_CIC>), grid, dim3(BLOCK), lds, h->stream, (const typename P::X*)x, mesh,
                         (typename P::W*)out, h->cfg.N, h->ld, h->cfg.Ng, h->cfg.L, h->dx);
  });
}

// indices and weights of `nenv` environments' worth of positions x [nenv][ld] -> idx, w [nenv][3][N]
void launch_shape_query(pic_handle* h, const void* x, int nenv, int shape, long long* idx, double* w) {
  const dim3 grid = aux_grid(h, nenv);
  with_format(h, [&](auto p) {
    using P = decltype(p);
    if (shape == PIC_TSC)
      hipLaunchKernelGGL((shape_query_kernel<P, PIC_TSC>), grid, dim3(BLOCK), 0, h->stream, (const typename P::X*)x, h->cfg.N,
                         h->ld, h->cfg.Ng, h->cfg.L, h->dx, idx, w);
    else
      hipLaunchKernelGGL((shape_query_kernel<P, PIC_CIC>), grid, dim3(BLOCK), 0, h->stream, (const typename P::X*)x, h->cfg.N,
                         h->ld, h->cfg.Ng, h->cfg.L, h->dx, idx, w);
  });
}

#include "host_diff.h"
#include "host_place.h"

}  // namespace

extern "C" {

int pic_abi_version(void) { return PICSTEP_ABI_VERSION; }

const char* pic_last_error(pic_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }


int pic_create(const pic_config* cfg, pic_handle** out) {
  if (!cfg || !out) return fail(nullptr, PIC_EINVAL, "pic_create: null argument");
  *out = nullptr;
  std::string err;
  if (int rc = check_config(*cfg, &err)) return fail(nullptr, rc, err);

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(nullptr, PIC_EHIP, "pic_create: no HIP device visible (this library has no CPU path)");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, PIC_EINVAL, "pic_create: bad device_id");
  {
    // the library holds gfx950 code objects only: say so here, not as hipErrorNoBinaryForGpu at the first launch
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device_id) != hipSuccess)
      return fail(nullptr, PIC_EHIP, "pic_create: hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(nullptr, PIC_EHIP, std::string("pic_create: device ") + std::to_string(cfg->device_id) + " is " + prop.gcnArchName +
                                         ": libpicstep.so is built for gfx950 (MI355X) only");
  }

  int ncu = 256;                             // (what the plan assumes of a device that does not say)
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device_id) != hipSuccess) ncu = 256;

  std::unique_ptr<pic_handle> owner(new (std::nothrow) pic_handle());     // a return before the end frees all the handle holds
  pic_handle* h = owner.get();
  if (!h) return fail(nullptr, PIC_ENOMEM, "pic_create: out of host memory");
  h->cfg = *cfg;
  if (int rc = plan_launch(*cfg, ncu, h, &err)) return fail(nullptr, rc, err);      // (host_plan.h: geometry, LDS, schedule)
  h->readonly_c = h->readonly_auto;
  h->alternate_stores = h->alternate_auto;
  const size_t stride = (size_t)cfg->Ng + 2;

  auto failed = [](hipError_t e, const char* what) {
    return fail(nullptr, e == hipErrorOutOfMemory ? PIC_ENOMEM : PIC_EHIP, std::string("pic_create: ") + what + ": " + hipGetErrorString(e));
  };
  if (hipError_t e = hipSetDevice(cfg->device_id)) return failed(e, "hipSetDevice");
  if (hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) return failed(e, "hipStreamCreateWithFlags");
  h->own_stream.reset(h->stream);
  const size_t pbytes = (size_t)cfg->num_envs * h->ld * h->esz;
  const size_t gbytes = (size_t)cfg->num_envs * cfg->Ng * sizeof(double);
  if (hipError_t e = alloc_particles(h, pbytes)) return failed(e, "allocation of the particles");     // x, v: [env][ld] each
  if (hipError_t e = hipMemsetAsync(h->x, 0, pbytes, h->stream)) return failed(e, "hipMemsetAsync of x");
  if (hipError_t e = hipMemsetAsync(h->v, 0, pbytes, h->stream)) return failed(e, "hipMemsetAsync of v");
  // small states (the reference's N = 5000) are read back every step by a Gym-style loop: one copy of x and v
  // together into pinned memory instead of two copies into pageable memory
  if (h->h_part_at_create)
    if (hipError_t e = alloc(h->h_part, 2 * (size_t)cfg->num_envs * h->ld * h->esz)) return failed(e, "pinned particle staging");
  if (hipError_t e = alloc_zeroed(h->ring, (size_t)(RING + 1) * h->S * gbytes, h->stream))      // acc_t and double are both 8 bytes
    return failed(e, "accumulator ring");
  h->probe_acc = ring_row(h, RING);
  if (h->resident) {
    const size_t qbytes = (size_t)cfg->num_envs * h->res_R * stride * sizeof(unsigned long long);
    if (hipError_t e = alloc_zeroed(h->res_q1, qbytes, h->stream)) return failed(e, "resident q1 meshes");
    // cells and weights of the q1 positions travel with it where a launch is latency, not traffic: a handful of environments
    // (20 bytes per particle each way: 256 environments would spend 8 us on them), kernels that carry them (pic_resident.h: kHandCarry)
    if (h->res_carry_bytes)
      if (hipError_t e = alloc_zeroed(h->res_carry, h->res_carry_bytes, h->stream)) return failed(e, "resident carried cells");
  }
  if (hipError_t e = alloc_zeroed(h->ke_part, (size_t)cfg->num_envs * h->nblk * sizeof(double), h->stream)) return failed(e, "KE partials");
  for (DeviceBuf<double>* g : {&h->n, &h->E_mesh, &h->phi, &h->ext, &h->ext2, &h->probe_ext, &h->aux_n, &h->aux_E, &h->aux_phi})
    if (hipError_t e = alloc_zeroed(*g, gbytes, h->stream)) return failed(e, "meshes");
  if (hipError_t e = alloc(h->e2, (size_t)cfg->num_envs * (cfg->Ng + 2) * sizeof(double))) return failed(e, "field tiles");
  // KE | PE | PE_reward live in one allocation so that a getter is a single small D2H copy into
  // pinned memory (a Python RL loop reads them every step)
  const size_t sbytes = (size_t)cfg->num_envs * sizeof(double);
  if (hipError_t e = alloc_zeroed(h->KE, 3 * sbytes, h->stream)) return failed(e, "energies");
  h->PE = h->KE + cfg->num_envs;
  h->PEr = h->KE + 2 * (size_t)cfg->num_envs;
  if (hipError_t e = alloc(h->h_scal, 3 * sbytes)) return failed(e, "pinned energy staging");
  if (h->LaunchPlan::h_fields)                 // (the plan's flag: the buffer of the same name hides it)
    if (hipError_t e = alloc(h->h_fields, 3 * gbytes)) return failed(e, "pinned mesh staging");
  if (hipError_t e = alloc(h->h_probe_pe, sbytes)) return failed(e, "pinned probe energy");
  if (hipError_t e = alloc_zeroed(h->aux_pe, sbytes, h->stream)) return failed(e, "probe energies");
  if (hipError_t e = alloc_zeroed(h->bad, 2 * sizeof(unsigned long long), h->stream)) return failed(e, "counters");
  h->probe_bad = h->bad + 1;
  if (hipError_t e = hipStreamSynchronize(h->stream)) return failed(e, "hipStreamSynchronize");
  *out = owner.release();
  return PIC_OK;
}

int pic_destroy(pic_handle* h) {
  if (!h) return PIC_OK;
  hipSetDevice(h->cfg.device_id);
  if (h->stream) hipStreamSynchronize(h->stream);
  prof_drain(h);
  delete h;
  return PIC_OK;
}

static int switch_stream(pic_handle* h, hipStream_t next) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));      // drain the old stream: later work must see its results
  prof_drain(h);
  h->stream = next;
  return PIC_OK;
}

int pic_set_stream(pic_handle* h, void* hip_stream) {
  if (!h) return PIC_EINVAL;
  return switch_stream(h, static_cast<hipStream_t>(hip_stream));      // NULL is a stream too: the device's default stream
}

int pic_own_stream(pic_handle* h) {
  if (!h) return PIC_EINVAL;
  return switch_stream(h, h->own_stream);
}

int pic_schedule(pic_handle* h) { return h ? (h->resident ? 1 : 0) : PIC_EINVAL; }

int pic_placement_info(pic_handle* h, int* candidates, double* kept_gbytes_per_s, double* slowest_gbytes_per_s,
                       double* seconds) {
  if (!h) return PIC_EINVAL;
  if (candidates) *candidates = h->place.pairs_timed > 0 ? h->place.pairs_timed : 1;
  if (kept_gbytes_per_s) *kept_gbytes_per_s = h->place.kept_gbytes_per_s;
  if (slowest_gbytes_per_s) *slowest_gbytes_per_s = h->place.slowest_gbytes_per_s;
  if (seconds) *seconds = h->place.seconds;
  return PIC_OK;
}

int pic_placement_stats(pic_handle* h, pic_placement* out) {
  if (!h || !out) return PIC_EINVAL;
  *out = h->place;
  return PIC_OK;
}

int pic_sync(pic_handle* h) {
  if (!h) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

int pic_set_particles(pic_handle* h, const void* x, const void* v, int mem_kind) {
  if (!h || !x || !v) return fail(h, PIC_EINVAL, "pic_set_particles: null argument");
  if (h->tape.on) return fail(h, PIC_ESTATE, "pic_set_particles: refused while a tape is open (pic_tape_stop first)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  drop_cached_deposits(h);      // first: an upload that fails half way has still changed x, and no cached deposit may outlive that
  int rc = upload_positions(h, h->x, x, mem_kind, h->bad);
  if (rc) return rc;
  rc = upload(h, h->v, v, mem_kind);
  if (rc) return rc;
  if (mem_kind == PIC_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  h->has_state = true;
  return PIC_OK;
}

int pic_invalidate(pic_handle* h) {
  if (!h) return PIC_EINVAL;
  drop_cached_deposits(h);
  return PIC_OK;
}

int pic_refresh(pic_handle* h) {
  if (!h) return PIC_EINVAL;
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_refresh: no particles loaded (call pic_reset first)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return refresh_fields(h);
}

int pic_reset(pic_handle* h, const void* x0, const void* v0, int mem_kind) {
  if (!h) return PIC_EINVAL;
  if (h->tape.on) return fail(h, PIC_ESTATE, "pic_reset: refused while a tape is open (pic_tape_stop first)");
  // (before resume_placement: a leg may move v, and a reset refused after that would leave garbage behind has_state)
  if (!x0 || !v0) return fail(h, PIC_EINVAL, "pic_set_particles: null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  resume_placement(h);
  HIPCHK(h, hipMemsetAsync(h->bad, 0, sizeof(unsigned long long), h->stream));
  int rc = pic_set_particles(h, x0, v0, mem_kind);
  if (rc) return rc;
  return refresh_fields(h);
}

// host -> device staging of a call's inputs.  Small per-step inputs have buffers of their own (h->ext, h->act); whole
// trajectories go through h->traj, grown on demand.
static int ensure_traj(pic_handle* h, size_t bytes) {
  if (bytes <= h->traj_bytes) return PIC_OK;
  const int rc = regrow(h, h->traj, bytes, "trajectory staging buffer");
  h->traj_bytes = rc ? 0 : bytes;
  return rc;
}

static int stage_ext(pic_handle* h, const double* E_ext, int mem_kind, const double** ext) {
  HIPCHK(h, device_input(h, E_ext, mem_kind, (size_t)h->cfg.num_envs * h->cfg.Ng * sizeof(double), h->ext, ext));
  return PIC_OK;
}

static int ensure_twiddle(pic_handle* h, int rows) {
  if (rows <= h->tw_rows) return PIC_OK;
  h->tw_rows = 0;
  const int rc = regrow(h, h->tw, (size_t)2 * rows * h->cfg.Ng * sizeof(double), "twiddle table");
  if (rc) return rc;
  hipLaunchKernelGGL(twiddle_kernel, dim3((h->cfg.Ng + BLOCK - 1) / BLOCK, rows), dim3(BLOCK), 0, h->stream, h->tw, h->cfg.Ng, rows);
  HIPCHK(h, hipGetLastError());
  h->tw_rows = rows;
  return PIC_OK;
}

// the shape of a call under `sc`, for the step schedule (host_schedule.h)
static CallShape call_shape(const pic_handle* h, const StepControl& sc) {
  CallShape p;
  p.scheme = h->scheme; p.cs = h->cs; p.ds = h->ds;
  p.light_inner_steps = h->light_inner_steps; p.readonly_c = h->readonly_c;
  p.alternate_stores = h->alternate_stores;
  p.feedback = sc.fb.M > 0; p.action = sc.ctl.act != nullptr;
  p.per_step_field = sc.ext_step != 0; p.per_step_action = sc.act_step != 0;
  return p;
}

// nsteps x PIC.update_state under `sc`, all launches enqueued, no host synchronisation.  hist: device [nsteps][3][env] record of
// the energies, or null; snap (resident schedule only): device record of the particles.
static int advance_steps(pic_handle* h, const StepControl& sc, int nsteps, double* hist, void* snap) {
  if (nsteps <= 0) return PIC_OK;
  const int E = h->cfg.num_envs;
  if (h->resident) {
    launch_resident(h, sc, nsteps, hist, snap);
    h->sched.drop_rows();            // the ring's q1 deposit belongs to the particles before these steps
    // the q1 mesh and the carried cells the kernel leaves behind are valid only if the launch went out: after a failed one the
    // next call must deposit q1 itself instead of taking over an unwritten block (the other integrators' kernel leaves none)
    const hipError_t e = launch_status(h);
    h->res_q1_valid = e == hipSuccess && h->scheme == PIC_YOSHIDA4;
    h->res_carry_valid = h->res_q1_valid && h->res_carry != nullptr;
    HIPCHK(h, e);
    return PIC_OK;
  }
  if (sc.fb.M > 0) {
    // The action of step s is the feedback law's on the field step s-1 left: the post-step solve is on the critical path
    // (a launch of its own that also computes the next action); before the first step a small kernel does it.
    Feedback fb = sc.fb;
    fb.act_out = h->act;
    hipLaunchKernelGGL(feedback_kernel, dim3(E), dim3(BLOCK), 0, h->stream, h->E_mesh, fb, h->cfg.Ng);
  }
  CallCtx cx;
  cx.sc = &sc; cx.hist = hist;
  plan_call(h->sched, call_shape(h, sc), nsteps, [&](const Launch& d) { run_launch(h, cx, d); });
  HIPCHK(h, launch_status(h));
  return PIC_OK;
}

// the two recorder kernels on the state as it stands (pic_record.h); appends one record
static int record_enqueue(pic_handle* h) {
  Recorder& r = h->rec;
  const int E = h->cfg.num_envs;
  const int64_t slot = (int64_t)r.steps.size();
  if (slot >= r.cap) return fail(h, PIC_ENOMEM, "the recorder is full");      // (every caller has checked: a last guard of the slot)
  RecordHistArgs ha{};
  ha.rec = r.u + (size_t)slot * E * r.u_stride;
  ha.u_stride = r.u_stride;
  ha.phase = r.phase;
  ha.xb = r.xb; ha.vb = r.vb; ha.px = r.px; ha.pv = r.pv;
  ha.phase_lds = r.plan.phase_lds;
  ha.rr = r.plan.rr;
  ha.N = h->cfg.N; ha.ld = h->ld; ha.tiles_per_wg = r.plan.tiles_per_wg;
  ha.L = h->cfg.L; ha.vmin = r.vmin; ha.vmax = r.vmax;
  // np.linspace steps: (stop - start) / div
  ha.sx = r.xb ? (h->cfg.L - 0.0) / r.xb : 0.0;
  ha.sv = r.vb ? (r.vmax - r.vmin) / r.vb : 0.0;
  ha.spx = r.px ? (h->cfg.L - 0.0) / r.px : 0.0;
  ha.spv = r.pv ? (r.vmax - r.vmin) / r.pv : 0.0;
  const dim3 grid(r.plan.gx, E);
  with_format(h, [&](auto p) {
    using P = decltype(p);
    hipLaunchKernelGGL(record_hist_kernel<P>, grid, dim3(BLOCK), r.plan.lds, h->stream, (const typename P::X*)h->x.get(),
                       (const typename P::V*)h->v, ha);
  });
  RecordFinishArgs fa{};
  fa.E_mesh = h->E_mesh; fa.KE = h->KE; fa.tw = h->tw; fa.tw_rows = h->tw_rows; fa.Ng = h->cfg.Ng; fa.M = r.M; fa.dx = h->dx;
  fa.rec = r.d + (size_t)slot * E * r.d_stride;
  fa.d_stride = r.d_stride;
  fa.phase = r.phase; fa.nb2 = r.px * r.pv; fa.feq = r.feq;
  fa.norm = r.px ? h->cfg.n0 / r.pdx / r.pdv / (double)h->cfg.N : 0.0;      // objective.py:12, left to right
  fa.dxdv = r.pdx * r.pdv;
  hipLaunchKernelGGL(record_finish_kernel, dim3(E), dim3(BLOCK), 0, h->stream, fa);
  HIPCHK(h, hipGetLastError());
  r.steps.push_back(r.k);
  return PIC_OK;
}

// records that nsteps more steps would add
static int64_t records_ahead(const pic_handle* h, int64_t nsteps) {
  const Recorder& r = h->rec;
  return r.on ? (r.k + nsteps) / r.stride - r.k / r.stride : 0;
}

// the host side of the differentiable rollouts (advance calls tape_record_ext, tape_checkpoint and tape_kl_enqueue)
#include "host_phase.h"
#include "host_moments.h"
#include "host_pool.h"
#include "host_tape.h"
#include "host_tangent.h"
#include "host_tangent_walk.h"
#include "host_copy.h"

// advance_steps, cut into parts where the recorder or an open tape needs the state between two steps.  A part runs up to the
// nearest of the next recorded step, the next checkpoint step (every step of a tape with a KL attached, pic_tape_kl_start) and
// the end of the call; such a step therefore ends like the last
// step of a call (full sweep D and a solve launch of its own; resident schedule: the end of a launch) -- stepping call by call
// gives the same bits.  Behind a part come the record kernels of a recorded step, then the tape's copy of the
// state after a checkpoint step.  Under a tape each part's external fields go on the tape first.
static int advance(pic_handle* h, const StepControl& sc, int nsteps, double* hist, void* snap = nullptr) {
  Recorder& r = h->rec;
  Tape& t = h->tape;
  const int E = h->cfg.num_envs;
  t.walk.on = t.twalk.on = t.policy.valid = false;   // appending abandons a walk (and dates the policy gradient of the last one)
  for (int done = 0; done < nsteps;) {
    int64_t n = nsteps - done;
    if (r.on) n = std::min<int64_t>(n, r.stride - r.k % r.stride);
    if (t.on) n = std::min<int64_t>(n, t.every - t.steps % t.every);
    if (t.on && (t.kl.on || t.mom_trace.trace)) n = 1;   // the KL or the moments (7l) of every step: the recorder's cut with stride 1
    const StepControl part = sc.after(done, E);
    int rc = t.on && part.fb.M == 0 ? tape_record_ext(h, part, (int)n) : PIC_OK;
    if (rc) return rc;
    rc = advance_steps(h, part, (int)n, hist_at(h, hist, done), snap_at(h, snap, done));
    if (rc) return rc;
    done += (int)n;
    if (r.on) {
      r.k += n;
      if (r.k % r.stride == 0) {
        rc = record_enqueue(h);
        if (rc) return rc;
      }
    }
    if (!t.on) continue;
    if (part.fb.M > 0) {
      // the gain law's actions exist only once their steps have run: e_t = B a_t from the actions the steps wrote on the tape
      // (pic_step_feedback_gain points act_hist at its rows)
      StepControl made{};
      made.ctl.basis = sc.ctl.basis; made.ctl.M = sc.ctl.M; made.ctl.act = part.fb.act_hist;
      made.act_step = (long long)E * 2 * sc.ctl.M;
      rc = tape_record_ext(h, made, (int)n);
      if (rc) return rc;
    }
    if (t.kl.on) {
      rc = tape_kl_enqueue(h);        // row t.steps of the trace
      if (rc) return rc;
    }
    if (t.mom_trace.trace) {
      rc = tape_moments_enqueue(h);   // row t.steps of the moments' trace
      if (rc) return rc;
    }
    t.steps += n;
    if (t.steps % t.every == 0) {
      rc = tape_checkpoint(h, t.steps / t.every);
      if (rc) return rc;
    }
  }
  return PIC_OK;
}

int pic_step_stage(pic_handle* h, int stage, const double* E_ext, int mem_kind) {
  if (!h) return PIC_EINVAL;
  if (h->tape.on) return fail(h, PIC_ESTATE, "pic_step_stage: refused while a tape is open (pic_tape_stop first)");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_step_stage: call pic_reset first");
  const int S = evals_per_step(h->scheme);
  if (stage < 1 || stage > S || stage != h->sched.mid_stage + 1)
    return fail(h, PIC_ESTATE, "pic_step_stage: stages run in the order 1.." + std::to_string(S) + " of the handle's integrator");
  if (stage == 1 && h->rec.on && (int64_t)h->rec.steps.size() + records_ahead(h, 1) > h->rec.cap)
    return fail(h, PIC_ENOMEM, "pic_step_stage: the step would take the recorder past its capacity");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  Control ctl{};
  int rc = stage_ext(h, E_ext, mem_kind, &ctl.ext);
  if (rc) return rc;
  h->res_q1_valid = false;           // (a resident handle steps by sweeps here: its carried q1 mesh goes stale)
  StepControl sc;
  sc.ctl = ctl;
  CallCtx cx;
  cx.sc = &sc;
  plan_stage(h->sched, call_shape(h, sc), stage, [&](const Launch& d) { run_launch(h, cx, d); });
  HIPCHK(h, hipGetLastError());
  if (stage == S && h->rec.on && ++h->rec.k % h->rec.stride == 0) return record_enqueue(h);
  return PIC_OK;
}

int pic_set_integrator(pic_handle* h, int scheme) {
  if (!h) return PIC_EINVAL;
  if (h->tape.on) return fail(h, PIC_ESTATE, "pic_set_integrator: refused while a tape is open (pic_tape_stop first)");
  if (scheme < PIC_YOSHIDA4 || scheme > PIC_FORWARD_EULER) return fail(h, PIC_EINVAL, "pic_set_integrator: unknown scheme");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, "pic_set_integrator: a staged step is in progress (finish its pic_step_stage calls)");
  if (scheme == h->scheme) return PIC_OK;
  drop_cached_deposits(h);           // the cached deposit belongs to a scheme (Yoshida-4: q1 = x + (c1 v) dt; the others: x)
  h->scheme = scheme;
  return PIC_OK;
}

int pic_set_readonly_c(pic_handle* h, int mode) {
  if (!h) return PIC_EINVAL;
  if (mode < PIC_READONLY_AUTO || mode > PIC_READONLY_ON) return fail(h, PIC_EINVAL, "pic_set_readonly_c: unknown mode");
  if (mode == PIC_READONLY_ON && !h->sweep_lds_rc)
    return fail(h, PIC_EINVAL, "pic_set_readonly_c: Ng too large for the second field tile of sweep D_RC");
  h->readonly_c = mode == PIC_READONLY_AUTO ? h->readonly_auto : mode == PIC_READONLY_ON;
  return PIC_OK;
}

int pic_set_alternate_stores(pic_handle* h, int mode) {
  if (!h) return PIC_EINVAL;
  if (mode < PIC_ALTERNATE_AUTO || mode > PIC_ALTERNATE_ON) return fail(h, PIC_EINVAL, "pic_set_alternate_stores: unknown mode");
  if (mode == PIC_ALTERNATE_ON && !h->sweep_lds_rc)
    return fail(h, PIC_EINVAL, "pic_set_alternate_stores: Ng too large for the second field tile of sweeps C_RB and B2_RD");
  h->alternate_stores = mode == PIC_ALTERNATE_AUTO ? h->alternate_auto : mode == PIC_ALTERNATE_ON;
  return PIC_OK;
}

int pic_get_integrator(pic_handle* h, int* scheme, int* evals) {
  if (!h) return PIC_EINVAL;
  if (scheme) *scheme = h->scheme;
  if (evals) *evals = evals_per_step(h->scheme);
  return PIC_OK;
}

static int check_steppable(pic_handle* h, int nsteps, const char* who) {
  if (!h->has_state) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_reset first");
  if (nsteps < 0) return fail(h, PIC_EINVAL, std::string(who) + ": nsteps < 0");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, std::string(who) + ": a staged step is in progress (finish its pic_step_stage calls)");
  if (h->rec.on && (int64_t)h->rec.steps.size() + records_ahead(h, nsteps) > h->rec.cap)
    return fail(h, PIC_ENOMEM, std::string(who) + ": the steps would take the recorder past its capacity (read and restart it, or "
                                                   "record with a larger capacity)");
  if (h->tape.on && h->tape.steps + nsteps > h->tape.max_steps)
    return fail(h, PIC_ENOMEM, std::string(who) + ": the steps would take the tape past max_steps (pic_tape_start)");
  return PIC_OK;
}

// The head of every stepping entry point: the handle, the entry point's own argument check (bad_args: what is wrong, or null),
// check_steppable, the device.  Nothing has been enqueued or changed when it fails.
static int step_prologue(pic_handle* h, int nsteps, const char* who, const char* bad_args = nullptr) {
  if (!h || bad_args) return fail(h, PIC_EINVAL, std::string(who) + ": " + (bad_args ? bad_args : "null argument"));
  int rc = check_steppable(h, nsteps, who);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return PIC_OK;
}

int pic_step(pic_handle* h, const double* E_ext, int mem_kind, int nsteps) {
  int rc = step_prologue(h, nsteps, "pic_step");
  if (rc) return rc;
  StepControl sc;
  rc = stage_ext(h, E_ext, mem_kind, &sc.ctl.ext);
  if (rc) return rc;
  return advance(h, sc, nsteps, nullptr);
}

// Runs `sc` for nsteps steps with the energies (hist, may be null) and / or the particles (snap, may be null) of every step
// kept on the device and read back once at the end; act_out (may be null): host [nsteps][env][2M] record of the feedback
// law's actions.  Returns after the read-backs, or -- nothing to read back -- without waiting for the device.
static int step_recording(pic_handle* h, StepControl sc, int nsteps, double* hist, void* snap, double* act_out, const char* who,
                          double* modes_out = nullptr) {
  if (nsteps == 0) return PIC_OK;
  const int E = h->cfg.num_envs;
  const size_t hbytes = (size_t)nsteps * 3 * E * sizeof(double);
  const size_t sbytes = (size_t)nsteps * 2 * E * (size_t)h->cfg.N * h->esz;
  const size_t abytes = (size_t)nsteps * E * 2 * sc.fb.M * sizeof(double);
  DeviceBuf<double> dh, da, dm;      // (freed at the return, behind the wait for the read-backs)
  DeviceBuf<void> ds;
  if (hist && alloc(dh, hbytes) != hipSuccess) return fail(h, PIC_ENOMEM, std::string(who) + ": history buffer");
  if (act_out && sc.fb.M > 0 && alloc(da, abytes) != hipSuccess) return fail(h, PIC_ENOMEM, std::string(who) + ": action record");
  if (modes_out && sc.fb.gain && alloc(dm, abytes) != hipSuccess) return fail(h, PIC_ENOMEM, std::string(who) + ": mode record");
  if (snap && alloc(ds, sbytes) != hipSuccess)
    return fail(h, PIC_ENOMEM, std::string(who) + ": the snapshots of all steps do not fit on the device; record fewer steps per call");
  if (da || !sc.fb.act_hist) sc.fb.act_hist = da;      // (pic_step_feedback_gain under a tape: the tape's rows)
  if (dm) sc.fb.modes_hist = dm;
  int rc = PIC_OK;
  if (!ds || h->resident) {
    rc = advance(h, sc, nsteps, dh, ds);      // energies: every post-step solve records its own entry; resident: the kernel records all
  } else {
    // particle snapshots on the streaming schedule: step by step, a copy kernel after each
    const dim3 grid = aux_grid(h, E);
    for (int s = 0; s < nsteps && rc == PIC_OK; ++s) {
      rc = advance(h, sc.after(s, E), 1, hist_at(h, dh, s));
      if (rc != PIC_OK) break;
      with_format(h, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL(record_particles_kernel<P>, grid, dim3(BLOCK), 0, h->stream, (const typename P::X*)h->x.get(),
                           (const typename P::V*)h->v, (typename P::V*)ds.get(), s, h->cfg.N, h->ld, h->cfg.L);
      });
    }
  }
  hipError_t e = hipGetLastError();
  const bool wait = dh || da || dm || ds;
  if (rc == PIC_OK && e == hipSuccess && dh) e = hipMemcpyAsync(hist, dh, hbytes, hipMemcpyDeviceToHost, h->stream);
  if (rc == PIC_OK && e == hipSuccess && da) e = hipMemcpyAsync(act_out, da, abytes, hipMemcpyDeviceToHost, h->stream);
  if (rc == PIC_OK && e == hipSuccess && dm) e = hipMemcpyAsync(modes_out, dm, abytes, hipMemcpyDeviceToHost, h->stream);
  if (rc == PIC_OK && e == hipSuccess && ds) e = hipMemcpyAsync(snap, ds, sbytes, hipMemcpyDeviceToHost, h->stream);
  if (rc != PIC_OK) {                 // (a failed step's error stands; what was enqueued is waited for)
    if (wait) (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  return hip_tail(h, e, wait, who);
}

// pic_step_history and pic_step_snapshots: a held field (or none), the energies and / or the particles of every step read back
static int step_held_recorded(pic_handle* h, const double* E_ext, int mem_kind, int nsteps, void* snap, double* hist,
                              const char* who, bool args_ok) {
  int rc = step_prologue(h, nsteps, who, args_ok ? nullptr : "null argument");
  if (rc) return rc;
  StepControl sc;
  rc = stage_ext(h, E_ext, mem_kind, &sc.ctl.ext);
  if (rc) return rc;
  return step_recording(h, sc, nsteps, hist, snap, nullptr, who);
}

int pic_step_history(pic_handle* h, const double* E_ext, int mem_kind, int nsteps, double* hist) {
  return step_held_recorded(h, E_ext, mem_kind, nsteps, nullptr, hist, "pic_step_history", hist != nullptr);
}

int pic_step_snapshots(pic_handle* h, const double* E_ext, int mem_kind, int nsteps, void* snap, double* hist) {
  return step_held_recorded(h, E_ext, mem_kind, nsteps, snap, hist, "pic_step_snapshots", snap != nullptr);
}

// a per-step input trajectory [nsteps][row] (host or device) -> device pointer
static int stage_traj(pic_handle* h, const double* src, int mem_kind, size_t row_elems_, int nsteps, const double** dev) {
  const size_t bytes = (size_t)nsteps * row_elems_ * sizeof(double);
  if (mem_kind == PIC_HOST)
    if (int rc = ensure_traj(h, bytes)) return rc;
  HIPCHK(h, device_input(h, src, mem_kind, bytes, static_cast<double*>(h->traj.get()), dev));
  return PIC_OK;
}

int pic_step_ext_traj(pic_handle* h, const double* E_ext_traj, int mem_kind, int nsteps, double* hist, void* snap) {
  int rc = step_prologue(h, nsteps, "pic_step_ext_traj", E_ext_traj ? nullptr : "null argument");
  if (rc) return rc;
  StepControl sc;
  sc.ext_step = (long long)h->cfg.num_envs * h->cfg.Ng;
  rc = stage_traj(h, E_ext_traj, mem_kind, (size_t)sc.ext_step, nsteps, &sc.ctl.ext);
  if (rc) return rc;
  return step_recording(h, sc, nsteps, hist, snap, nullptr, "pic_step_ext_traj");
}

// x | v rows (and, with scalars, KE | PE | PE_reward) of float-position handles into the pinned staging buffers; the caller
// synchronises.  Up to kTinyState bytes a kernel of the handle's stream writes them (a copy command costs 5-7 us of launch
// latency behind a 20 us step, a kernel that stores to pinned memory 2.6: profiles/d2h_probe.hip); larger states go by copy
// commands (stores over PCIe run at ~9 GB/s from a kernel, the copy engine at ~50).  The staging for x | v exists from
// pic_create on for states up to 4 MB and is made here, once, for states up to 64 MB (a vectorised host-side loop over tens
// of environments: 64 x N = 5000 read back in 0.4 instead of 1.4 ms).
constexpr size_t kTinyState = (size_t)512 << 10;
static bool ensure_part_staging(pic_handle* h) {
  const size_t total = 2 * (size_t)h->cfg.num_envs * h->ld * h->esz;      // rows as they lie on the device (padded to ld)
  if (!h->h_part && !h->h_part_refused && total <= ((size_t)64 << 20)) {
    if (alloc(h->h_part, total) != hipSuccess) {
      h->h_part_refused = true;
      (void)hipGetLastError();
    }
  }
  return h->h_part != nullptr;
}
// *pitch: bytes from one environment's row to the next in the staging buffer (x rows, then v rows)
static int enqueue_observe(pic_handle* h, bool scalars, size_t* pitch) {
  const int E = h->cfg.num_envs;
  const size_t row = (size_t)h->cfg.N * h->esz;
  *pitch = row;
  if (2 * row * E > kTinyState || 2 * E > 65535) {      // (the kernel below numbers environments in grid.y: at most 65535 rows)
    // the arrays as they lie on the device, padding included, in plain copies (a strided copy command runs at a seventh of the rate)
    const size_t block = (size_t)E * h->ld * h->esz;
    *pitch = (size_t)h->ld * h->esz;
    if (!h->v_separate) {
      HIPCHK(h, hipMemcpyAsync(h->h_part, h->x, 2 * block, hipMemcpyDeviceToHost, h->stream));
    } else {
      HIPCHK(h, hipMemcpyAsync(h->h_part, h->x, block, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpyAsync(static_cast<char*>(h->h_part.get()) + block, h->v, block, hipMemcpyDeviceToHost, h->stream));
    }
    if (scalars) HIPCHK(h, hipMemcpyAsync(h->h_scal, h->KE, 3 * (size_t)E * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return PIC_OK;
  }
  dim3 grid((unsigned)std::min<long long>((h->cfg.N + BLOCK - 1) / BLOCK, 64), 2 * E);
  if (h->esz == 8)
    hipLaunchKernelGGL(observe_kernel<double>, grid, dim3(BLOCK), 0, h->stream, static_cast<const double*>(h->x.get()),
                       static_cast<const double*>(h->v), (long long)h->cfg.N, (long long)h->ld, E, static_cast<double*>(h->h_part.get()),
                       h->KE, scalars ? h->h_scal : nullptr);
  else
    hipLaunchKernelGGL(observe_kernel<float>, grid, dim3(BLOCK), 0, h->stream, static_cast<const float*>(h->x.get()),
                       static_cast<const float*>(h->v), (long long)h->cfg.N, (long long)h->ld, E, static_cast<float*>(h->h_part.get()),
                       h->KE, scalars ? h->h_scal : nullptr);
  HIPCHK(h, hipGetLastError());
  return PIC_OK;
}
// x and v (either may be null) on their way to the caller, enqueued; the caller waits.  staged: through the pinned staging, rows
// *pitch bytes apart (unpack_part behind the wait; the two callers differ in when they stage), else straight into x and v in
// mem_kind's memory.  scalars: the energies travel along, into h_scal.
static int enqueue_particles_out(pic_handle* h, void* x, void* v, int mem_kind, bool staged, bool scalars, size_t* pitch) {
  if (staged) return enqueue_observe(h, scalars, pitch);
  if (scalars) HIPCHK(h, hipMemcpyAsync(h->h_scal, h->KE, 3 * (size_t)h->cfg.num_envs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  int rc = PIC_OK;
  if (x) rc = download_positions(h, x, h->x, mem_kind);
  if (!rc && v) rc = download(h, v, h->v, mem_kind);
  return rc;
}
// staging -> the caller's [num_envs][N] arrays
static void unpack_part(pic_handle* h, void* x, void* v, size_t pitch) {
  const size_t E = (size_t)h->cfg.num_envs, row = (size_t)h->cfg.N * h->esz;
  const char* sx = static_cast<const char*>(h->h_part.get());
  const char* sv = sx + E * pitch;
  if (pitch == row) {
    if (x) std::memcpy(x, sx, E * row);
    if (v) std::memcpy(v, sv, E * row);
    return;
  }
  for (size_t e = 0; e < E; ++e) {
    if (x) std::memcpy(static_cast<char*>(x) + e * row, sx + e * pitch, row);
    if (v) std::memcpy(static_cast<char*>(v) + e * row, sv + e * pitch, row);
  }
}

// Actuator coefficients of one call, given on the host, to where the step reads them.  A handful (one environment's action:
// <= kInlineDoubles) rides in the argument blocks of the kernels that use it -- the resident kernel's, or the three sweeps' --
// where a pageable host-to-device copy command, or a launch of its own, costs 5-6 us on the stream in front of the step.
static int stage_actions(pic_handle* h, const double* actions, StepControl& sc) {
  const int n = h->cfg.num_envs * 2 * h->act_modes;
  sc.ctl.act = h->act;
  if (n <= kInlineDoubles) {
    std::memcpy(sc.inline_act.v, actions, (size_t)n * sizeof(double));
    sc.inline_n = n;
    return PIC_OK;
  }
  HIPCHK(h, hipMemcpyAsync(h->act, actions, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return PIC_OK;
}

int pic_get_particles(pic_handle* h, void* x, void* v, int mem_kind) {
  if (!h) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  // states up to 64 MB go through pinned staging (enqueue_observe)
  const bool staged = x && v && mem_kind == PIC_HOST && h->fmt != FMT_U32 && ensure_part_staging(h);
  size_t pitch = 0;
  const int rc = enqueue_particles_out(h, x, v, mem_kind, staged, false, &pitch);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (staged) unpack_part(h, x, v, pitch);
  return PIC_OK;
}

int pic_device_ptrs(pic_handle* h, void** x, void** v, int64_t* ld, double** n, double** E_mesh, double** phi,
                    double** KE, double** PE, double** PE_reward) {
  if (!h) return PIC_EINVAL;
  if (x || v) h->place_state.ptrs_exposed = true;       // (from here on the search for a placement may not move v: resume_placement)
  if (x) *x = h->x;
  if (v) *v = h->v;
  if (ld) *ld = h->ld;
  if (n) *n = h->n;
  if (E_mesh) *E_mesh = h->E_mesh;
  if (phi) *phi = h->phi;
  if (KE) *KE = h->KE;
  if (PE) *PE = h->PE;
  if (PE_reward) *PE_reward = h->PEr;
  return PIC_OK;
}

int pic_get_fields(pic_handle* h, double* n, double* E_mesh, double* phi) {
  if (!h) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t gbytes = (size_t)h->cfg.num_envs * h->cfg.Ng * sizeof(double);
  if (h->h_fields) {                                  // small meshes: one kernel writes all three into pinned memory, one wait
    const long long count = (long long)h->cfg.num_envs * h->cfg.Ng;
    hipLaunchKernelGGL(fields_out_kernel, dim3((unsigned)std::min<long long>((count + BLOCK - 1) / BLOCK, 64), 3), dim3(BLOCK), 0,
                       h->stream, h->n, h->E_mesh, h->phi, h->h_fields, count);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n) std::memcpy(n, h->h_fields, gbytes);
    if (E_mesh) std::memcpy(E_mesh, h->h_fields + count, gbytes);
    if (phi) std::memcpy(phi, h->h_fields + 2 * count, gbytes);
    return PIC_OK;
  }
  HIPCHK(h, read_back(h, gbytes, {{n, h->n}, {E_mesh, h->E_mesh}, {phi, h->phi}}));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

int pic_get_energies(pic_handle* h, double* KE, double* PE, double* PE_reward) {
  if (!h) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipMemcpyAsync(h->h_scal, h->KE, 3 * (size_t)h->cfg.num_envs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unpack_scalars(h, KE, PE, PE_reward);
  return PIC_OK;
}

static int ensure_scratch(pic_handle* h) {
  if (h->scratch) return PIC_OK;
  const size_t pbytes = (size_t)h->cfg.num_envs * h->ld * h->esz;
  HIPCHK(h, alloc_zeroed(h->scratch, pbytes, h->stream));
  return PIC_OK;
}

int pic_gather_E(pic_handle* h, void* E_particles, int mem_kind) {
  if (!h || !E_particles) return fail(h, PIC_EINVAL, "pic_gather_E: null argument");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_gather_E: call pic_reset first");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  void* dst = E_particles;
  if (mem_kind == PIC_HOST) {
    int rc = ensure_scratch(h);
    if (rc) return rc;
    dst = h->scratch;     // dense [env][N] fits in [env][ld]
  }
  launch_gather(h, h->x, h->E_mesh, dst);
  HIPCHK(h, hipGetLastError());
  if (mem_kind == PIC_HOST)
    HIPCHK(h, hipMemcpyAsync(E_particles, dst, (size_t)h->cfg.num_envs * h->cfg.N * h->esz, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

int pic_get_cic(pic_handle* h, int env, int64_t* indx_l, int64_t* indx_r, double* weight_l, double* weight_r) {
  if (!h) return PIC_EINVAL;
  if (env < 0 || env >= h->cfg.num_envs) return fail(h, PIC_EINVAL, "pic_get_cic: env out of range");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_get_cic: call pic_reset first");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const long long N = h->cfg.N;
  DeviceBuf<long long> dj;
  DeviceBuf<double> dw;
  HIPCHK(h, alloc(dj, 3 * N * sizeof(long long)));
  if (alloc(dw, 3 * N * sizeof(double)) != hipSuccess) return fail(h, PIC_ENOMEM, "pic_get_cic: hipMalloc");
  const char* xe = (const char*)h->x.get() + (size_t)env * h->ld * h->esz;
  launch_shape_query(h, xe, 1, PIC_CIC, dj, dw);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && indx_l) e = hipMemcpyAsync(indx_l, dj, N * sizeof(long long), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && indx_r) e = hipMemcpyAsync(indx_r, dj + N, N * sizeof(long long), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && weight_l) e = hipMemcpyAsync(weight_l, dw, N * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && weight_r) e = hipMemcpyAsync(weight_r, dw + N, N * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  return hip_tail(h, e, true, "pic_get_cic");
}

// deposit of the positions in h->scratch into the probe accumulator, then one solve with `ext` added
// Deposit + solve of the positions at `xs` ([env][ld], device-readable: h->scratch, or pinned host memory) into the aux meshes.
// pe_out: where the solve leaves 0.5 sum(E^2) dx per environment (h->aux_pe, or pinned host memory).
static int probe_solve(pic_handle* h, const double* E_ext, bool want_phi, void* xs = nullptr, double* pe_out = nullptr) {
  const size_t gbytes = (size_t)h->cfg.num_envs * h->cfg.Ng * sizeof(double);
  const double* ext = nullptr;
  HIPCHK(h, device_input(h, E_ext, PIC_HOST, gbytes, h->probe_ext, &ext));
  if (!xs) xs = h->scratch;
  // (the solve zeroes the row behind its read: one command less per probe; a probe that failed half way leaves it unknown)
  if (!h->probe_row_clean) HIPCHK(h, hipMemsetAsync(h->probe_acc, 0, row_elems(h) * sizeof(acc_t), h->stream));
  h->probe_row_clean = false;
  CallCtx cx;
  cx.probe_x = xs;
  plan_probe(h->sched, [&](const Launch& d) { run_launch(h, cx, d); });
  SolveIO o{};
  o.acc = h->probe_acc; o.acc_clear = h->probe_acc; o.out.ext = ext; o.n = h->aux_n; o.out.E = h->aux_E;
  o.out.PEr = pe_out ? pe_out : h->aux_pe;
  if (want_phi) o.out.phi = h->aux_phi;
  launch_solve(h, o);
  HIPCHK(h, hipGetLastError());
  h->probe_row_clean = true;
  return PIC_OK;
}

int pic_eval_field(pic_handle* h, const void* x, int mem_kind, const double* E_ext, double* n, double* E_mesh,
                   double* half_sum_E2_dx) {
  if (!h || !x) return fail(h, PIC_EINVAL, "pic_eval_field: null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t gbytes = (size_t)h->cfg.num_envs * h->cfg.Ng * sizeof(double);
  const size_t E = (size_t)h->cfg.num_envs, row = (size_t)h->cfg.N * h->esz;
  // A small host state (Reward.compute_reward of a trainer that only changed its imports: reward.py:48-50, once per step): the
  // positions go into the pinned staging buffer with a host copy and the probe sweep reads them from there, the solve writes
  // the energy into pinned memory -- two kernels and one wait instead of seven commands (78 -> 3x us per call at N = 5000).
  if (mem_kind == PIC_HOST && h->fmt != FMT_U32 && E * row <= kTinyState / 2 && ensure_part_staging(h)) {
    const size_t pitch = (size_t)h->ld * h->esz;
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (the staging buffer may still be the target of an earlier read-back)
    for (size_t e = 0; e < E; ++e) {
      char* dst = static_cast<char*>(h->h_part.get()) + e * pitch;
      std::memcpy(dst, static_cast<const char*>(x) + e * row, row);
      std::memset(dst + row, 0, pitch - row);
    }
    int rc = probe_solve(h, E_ext, false, h->h_part, h->h_probe_pe);
    if (rc) return rc;
    HIPCHK(h, read_back(h, gbytes, {{n, h->aux_n}, {E_mesh, h->aux_E}}));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (half_sum_E2_dx) std::memcpy(half_sum_E2_dx, h->h_probe_pe, E * sizeof(double));
    return PIC_OK;
  }
  int rc = ensure_scratch(h);
  if (rc) return rc;
  rc = upload_positions(h, h->scratch, x, mem_kind, h->probe_bad);
  if (rc) return rc;
  rc = probe_solve(h, E_ext, false);
  if (rc) return rc;
  HIPCHK(h, read_back(h, gbytes, {{n, h->aux_n}, {E_mesh, h->aux_E}}));
  if (half_sum_E2_dx)
    HIPCHK(h, hipMemcpyAsync(half_sum_E2_dx, h->aux_pe, (size_t)h->cfg.num_envs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

int pic_compute_E(pic_handle* h, const void* x, int mem_kind, const double* E_ext, void* E_part, void* phi_part,
                  double* n, double* E_mesh, double* phi_mesh, int64_t* idx, double* w) {
  if (!h || !x) return fail(h, PIC_EINVAL, "pic_compute_E: null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  int rc = ensure_scratch(h);
  if (rc) return rc;
  rc = upload_positions(h, h->scratch, x, mem_kind, h->probe_bad);
  if (rc) return rc;
  const int E_ = h->cfg.num_envs;
  const long long N = h->cfg.N;
  const size_t gbytes = (size_t)E_ * h->cfg.Ng * sizeof(double);
  rc = probe_solve(h, E_ext, true);
  if (rc) return rc;
  HIPCHK(h, read_back(h, gbytes, {{n, h->aux_n}, {E_mesh, h->aux_E}, {phi_mesh, h->aux_phi}}));

  // gathers at the particles and shape bookkeeping go through one temporary, sized for the larger of the two
  DeviceBuf<void> tmp;
  const size_t part_bytes = (size_t)E_ * N * h->esz;
  const size_t shape_bytes = (size_t)E_ * 3 * N * 8;
  const bool want_shape = idx || w;
  if (E_part || phi_part || want_shape) {
    if (alloc(tmp, want_shape ? 2 * shape_bytes : part_bytes) != hipSuccess)
      return fail(h, PIC_ENOMEM, "pic_compute_E: hipMalloc of the gather buffer");
  }
  hipError_t e = hipSuccess;
  const double* meshes[2] = {h->aux_E, h->aux_phi};
  void* outs[2] = {E_part, phi_part};
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    if (!outs[k]) continue;
    launch_gather(h, h->scratch, meshes[k], tmp);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(outs[k], tmp, part_bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);      // tmp is reused
  }
  if (want_shape && e == hipSuccess) {
    long long* dj = static_cast<long long*>(tmp.get());
    double* dw = reinterpret_cast<double*>(static_cast<char*>(tmp.get()) + shape_bytes);
    launch_shape_query(h, h->scratch, E_, h->cfg.interpol, dj, dw);
    e = hipGetLastError();
    if (e == hipSuccess && idx) e = hipMemcpyAsync(idx, dj, shape_bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && w) e = hipMemcpyAsync(w, dw, shape_bytes, hipMemcpyDeviceToHost, h->stream);
  }
  return hip_tail(h, e, true, "pic_compute_E");
}

int pic_solve_poisson(pic_handle* h, const double* rhs, double* phi, double* E_mesh) {
  if (!h || !rhs) return fail(h, PIC_EINVAL, "pic_solve_poisson: null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t gbytes = (size_t)h->cfg.num_envs * h->cfg.Ng * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(h->aux_n, rhs, gbytes, hipMemcpyHostToDevice, h->stream));
  SolveIO o{};
  o.rhs = h->aux_n; o.out.E = h->aux_E; o.out.phi = h->aux_phi;
  launch_solve(h, o);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, read_back(h, gbytes, {{phi, h->aux_phi}, {E_mesh, h->aux_E}}));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

int pic_set_actuator(pic_handle* h, int max_mode, const double* basis_cos, const double* basis_sin) {
  if (!h || !basis_cos || !basis_sin || max_mode < 1 || max_mode > 64)
    return fail(h, PIC_EINVAL, "pic_set_actuator: need 1 <= max_mode <= 64 and both basis tables");
  if (h->tape.on) return fail(h, PIC_ESTATE, "pic_set_actuator: refused while a tape is open (pic_tape_stop first)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  h->act_modes = 0;                      // (until both tables are in place)
  const size_t tb = (size_t)h->cfg.Ng * max_mode * sizeof(double);
  int rc = regrow(h, h->basis, 2 * tb, "pic_set_actuator: the basis tables do not fit on the device");
  if (!rc) rc = regrow(h, h->act, (size_t)h->cfg.num_envs * 2 * max_mode * sizeof(double), "pic_set_actuator: the actions do not fit on the device");
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(h->basis, basis_cos, tb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync((char*)h->basis.get() + tb, basis_sin, tb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->act_modes = max_mode;
  return PIC_OK;
}

static int actuator_control(pic_handle* h, StepControl& sc, const char* who) {
  if (!h->act_modes) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_set_actuator first");
  sc.ctl.basis = h->basis;
  sc.ctl.M = h->act_modes;
  return PIC_OK;
}

// The feedback law of a call (pic_step_feedback, pic_step_feedback_gain) on the actuator's modes, with their twiddles (a call of
// no steps checks and makes none)
static int feedback_control(pic_handle* h, int max_mode, int nsteps, StepControl& sc, const char* who) {
  int rc = actuator_control(h, sc, who);
  if (rc) return rc;
  if (max_mode != h->act_modes || max_mode > kMaxFeedbackModes)
    return fail(h, PIC_EINVAL, std::string(who) + ": max_mode must equal the actuator's (pic_set_actuator) and be at most 16");
  if (nsteps == 0) return PIC_OK;
  rc = ensure_twiddle(h, max_mode);
  if (rc) return rc;
  sc.fb.tw = h->tw; sc.fb.rows = h->tw_rows; sc.fb.M = max_mode;
  sc.fb.act_out = h->act;
  return PIC_OK;
}

int pic_step_actions(pic_handle* h, const double* actions, int mem_kind, int nsteps) {
  int rc = step_prologue(h, nsteps, "pic_step_actions", actions ? nullptr : "null argument");
  if (rc) return rc;
  StepControl sc;
  rc = actuator_control(h, sc, "pic_step_actions");
  if (rc) return rc;
  sc.ctl.act = actions;
  if (mem_kind == PIC_HOST) {
    rc = stage_actions(h, actions, sc);
    if (rc) return rc;
  }
  return advance(h, sc, nsteps, nullptr);
}

int pic_step_observe(pic_handle* h, const double* E_ext, const double* actions, int nsteps, void* x, void* v, double* KE,
                     double* PE, double* PE_reward) {
  int rc = step_prologue(h, nsteps, "pic_step_observe", E_ext && actions ? "E_ext and actions are alternatives" : nullptr);
  if (rc) return rc;
  StepControl sc;
  if (actions) {
    rc = actuator_control(h, sc, "pic_step_observe");
    if (rc) return rc;
    rc = stage_actions(h, actions, sc);
    if (rc) return rc;
  } else {
    rc = stage_ext(h, E_ext, PIC_HOST, &sc.ctl.ext);
    if (rc) return rc;
  }
  // Everything the caller reads goes into pinned memory behind the step, then ONE wait.  Small states have pinned staging
  // (h_part).  A one-step call of the resident schedule needs nothing else: its kernel records the particles after the step
  // (the snapshot of PIC.simulate, positions in length units whatever their format) and the step's energies (the energy
  // history) -- both straight into the pinned buffers, whose layouts are those records' for one step.
  const size_t row = (size_t)h->cfg.N * h->esz, half = row * (size_t)h->cfg.num_envs;
  const bool want_part = x || v;
  bool part_pinned = false;
  size_t pitch = row;
  if (want_part) ensure_part_staging(h);
  if (h->resident && nsteps == 1 && h->h_part && 2 * half <= kTinyState) {
    rc = advance(h, sc, 1, h->h_scal, want_part ? h->h_part : nullptr);
    if (rc) return rc;
    part_pinned = want_part;
  } else {
    rc = advance(h, sc, nsteps, nullptr);
    if (rc) return rc;
    part_pinned = want_part && h->h_part && h->fmt != FMT_U32;
    rc = enqueue_particles_out(h, x, v, PIC_HOST, part_pinned, true, &pitch);
    if (rc) return rc;
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (part_pinned) unpack_part(h, x, v, pitch);
  unpack_scalars(h, KE, PE, PE_reward);
  return PIC_OK;
}

int pic_step_actions_traj(pic_handle* h, const double* actions, int mem_kind, int nsteps, double* hist) {
  int rc = step_prologue(h, nsteps, "pic_step_actions_traj", actions ? nullptr : "null argument");
  if (rc) return rc;
  StepControl sc;
  rc = actuator_control(h, sc, "pic_step_actions_traj");
  if (rc) return rc;
  sc.act_step = (long long)h->cfg.num_envs * 2 * h->act_modes;
  rc = stage_traj(h, actions, mem_kind, (size_t)sc.act_step, nsteps, &sc.ctl.act);
  if (rc) return rc;
  return step_recording(h, sc, nsteps, hist, nullptr, nullptr, "pic_step_actions_traj");
}

int pic_step_feedback(pic_handle* h, int max_mode, int nsteps, double* actions_out, double* hist) {
  if (h && h->tape.on)
    return fail(h, PIC_ESTATE, "pic_step_feedback: refused while a tape is open (its actions depend on the state: the gradient through the law would be missing)");
  int rc = step_prologue(h, nsteps, "pic_step_feedback");
  if (rc) return rc;
  StepControl sc;
  rc = feedback_control(h, max_mode, nsteps, sc, "pic_step_feedback");
  if (rc) return rc;
  return step_recording(h, sc, nsteps, hist, nullptr, actions_out, "pic_step_feedback");
}

int pic_step_feedback_gain(pic_handle* h, int max_mode, const double* gain, int mem_kind, int nsteps, double* actions_out,
                           double* modes_out, double* hist) {
  const char* who = "pic_step_feedback_gain";
  int rc = step_prologue(h, nsteps, who, !gain ? "null gain" : (mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) ? "bad mem_kind" : nullptr);
  if (rc) return rc;
  StepControl sc;
  rc = feedback_control(h, max_mode, nsteps, sc, who);
  if (rc || nsteps == 0) return rc;
  const int E = h->cfg.num_envs, n = 2 * max_mode;
  const size_t gbytes = (size_t)E * n * n * sizeof(double);
  if (!h->fb_modes) HIPCHK(h, alloc(h->fb_modes, (size_t)E * 2 * kMaxFeedbackModes * sizeof(double)));
  Tape& t = h->tape;
  const double* g = gain;
  if (t.on) {                        // the gain goes on the tape once per call
    rc = tape_law_reserve(h, gbytes);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(t.law.gains.back(), gain, gbytes, copy_kind(mem_kind, hipMemcpyHostToDevice), h->stream));
    g = t.law.gains.back();
  } else {
    if (mem_kind == PIC_HOST && !h->gain) HIPCHK(h, alloc(h->gain, (size_t)E * 4 * kMaxFeedbackModes * kMaxFeedbackModes * sizeof(double)));
    HIPCHK(h, device_input(h, gain, mem_kind, gbytes, h->gain, &g));
  }
  sc.fb.gain = g;
  sc.fb.modes = h->fb_modes;
  if (!t.on) return step_recording(h, sc, nsteps, hist, nullptr, actions_out, who, modes_out);
  // taped: the steps write their actions and modes on the tape, the caller's records are copied from there
  const int64_t s0 = t.steps;
  const size_t row = (size_t)E * n;
  sc.fb.act_hist = t.law.act + (size_t)s0 * row;
  sc.fb.modes_hist = t.law.modes + (size_t)s0 * row;
  rc = step_recording(h, sc, nsteps, hist, nullptr, nullptr, who);
  for (int64_t s = s0; s < t.steps; ++s) t.law.step[(size_t)s] = (int)t.law.gains.size() - 1;
  if (rc) return rc;
  if (actions_out) HIPCHK(h, hipMemcpyAsync(actions_out, sc.fb.act_hist, (size_t)nsteps * row * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (modes_out) HIPCHK(h, hipMemcpyAsync(modes_out, sc.fb.modes_hist, (size_t)nsteps * row * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (actions_out || modes_out) HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

// what a controller call has in common, then closed loops under an MLP policy (pic_policy_eval, pic_step_policy)
#include "host_head.h"
#include "host_policy.h"
// ... and under the DeepSets particle actor (pic_actor_eval, pic_step_actor)
#include "host_actor.h"

int pic_get_modes(pic_handle* h, int max_mode, double* re, double* im, int mem_kind) {
  if (!h || max_mode < 1 || max_mode >= h->cfg.Ng) return fail(h, PIC_EINVAL, "pic_get_modes: bad max_mode");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_get_modes: call pic_reset first");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t nb = (size_t)h->cfg.num_envs * max_mode * sizeof(double);
  int rc = PIC_OK;
  if (max_mode > h->modes_cap) {          // (re)allocate only when a larger mode count is asked for
    h->modes_cap = 0;
    rc = regrow(h, h->modes, 2 * nb, "pic_get_modes: the modes do not fit on the device");
    if (rc) return rc;
    h->modes_cap = max_mode;
  }
  rc = ensure_twiddle(h, max_mode);
  if (rc) return rc;
  double* dre = h->modes;
  double* dim_ = h->modes + (size_t)h->cfg.num_envs * max_mode;
  hipLaunchKernelGGL(modes_kernel, dim3(max_mode, h->cfg.num_envs), dim3(BLOCK), 0, h->stream, h->E_mesh, h->tw, h->tw_rows,
                     dre, dim_, h->cfg.Ng, max_mode);
  HIPCHK(h, hipGetLastError());
  const hipMemcpyKind k = copy_kind(mem_kind, hipMemcpyDeviceToHost);
  if (re) HIPCHK(h, hipMemcpyAsync(re, dre, nb, k, h->stream));
  if (im) HIPCHK(h, hipMemcpyAsync(im, dim_, nb, k, h->stream));
  if (mem_kind == PIC_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));   // device outputs stay stream-ordered
  return PIC_OK;
}

int pic_reset_sampled(pic_handle* h, int kind, double a, double v0, double sigma, double A, int n_mode,
                      uint64_t seed) {
  if (!h || (kind != 0 && kind != 1) || !(sigma > 0) || (kind == 1 && !(a >= 0)))
    return fail(h, PIC_EINVAL, "pic_reset_sampled: kind must be 0 (two-stream) or 1 (bump-on-tail), sigma > 0, a >= 0");
  // the reference accepts with u < pdf(v) (dist.py:66-68): where the peak 1/sqrt(2 pi)/sigma exceeds 1 its density is
  // min(pdf, 1), a clipped Gaussian this sampler does not draw
  if (1.0 / sqrt(2.0 * M_PI) / sigma > 1.0)
    return fail(h, PIC_EINVAL, "pic_reset_sampled: sigma < 1/sqrt(2 pi) (the reference's density is clipped there): "
                               "draw on the host (env.dist) and pass the sample to pic_reset");
  if (h->tape.on) return fail(h, PIC_ESTATE, "pic_reset_sampled: refused while a tape is open (pic_tape_stop first)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  resume_placement(h);
  const dim3 grid = aux_grid(h, h->cfg.num_envs, 2048);
  with_format(h, [&](auto p) {
    using P = decltype(p);
    hipLaunchKernelGGL(sample_kernel<P>, grid, dim3(BLOCK), 0, h->stream, (typename P::X*)h->x.get(), (typename P::V*)h->v, h->cfg.N,
                       h->ld, kind, a, v0, sigma, A, n_mode, h->cfg.L, (unsigned long long)seed, h->cfg.env_index_base);
  });
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemsetAsync(h->bad, 0, sizeof(unsigned long long), h->stream));
  h->has_state = true;
  return refresh_fields(h);      // a reset abandons an open staged step and any cached deposit
}

// counts[num_envs][nbins][nbins] of the current particles into a fresh device buffer d
static hipError_t phase_counts(pic_handle* h, int nbins, double vmin, double vmax, DeviceBuf<unsigned>& d) {
  const size_t nb = (size_t)h->cfg.num_envs * nbins * nbins * sizeof(unsigned);
  hipError_t e = alloc_zeroed(d, nb, h->stream);
  const dim3 grid = aux_grid(h, h->cfg.num_envs, 2048);
  if (e == hipSuccess) {
    with_format(h, [&](auto p) {
      using P = decltype(p);
      hipLaunchKernelGGL(phase_hist_kernel<P>, grid, dim3(BLOCK), 0, h->stream, (const typename P::X*)h->x.get(),
                         (const typename P::V*)h->v, d, h->cfg.N, h->ld, nbins, h->cfg.L, vmin, vmax);
    });
    e = hipGetLastError();
  }
  return e;
}

int pic_phase_histogram(pic_handle* h, int nbins, double vmin, double vmax, uint32_t* counts) {
  if (!h || !counts || nbins < 1 || nbins > 4096 || !(vmax > vmin))
    return fail(h, PIC_EINVAL, "pic_phase_histogram: need counts, 1 <= nbins <= 4096, vmax > vmin");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_phase_histogram: call pic_reset first");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t nb = (size_t)h->cfg.num_envs * nbins * nbins * sizeof(unsigned);
  DeviceBuf<unsigned> d;
  hipError_t e = phase_counts(h, nbins, vmin, vmax, d);
  if (e == hipSuccess) e = hipMemcpyAsync(counts, d, nb, hipMemcpyDeviceToHost, h->stream);
  return hip_tail(h, e, true, "pic_phase_histogram");
}

int pic_phase_kl(pic_handle* h, int nbins, double vmin, double vmax, const double* feq, double* kl) {
  if (!h || !feq || !kl || nbins < 1 || nbins > 4096 || !(vmax > vmin))
    return fail(h, PIC_EINVAL, "pic_phase_kl: need feq, kl, 1 <= nbins <= 4096, vmax > vmin");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_phase_kl: call pic_reset first");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int E = h->cfg.num_envs, nb2 = nbins * nbins;
  DeviceBuf<unsigned> d;
  DeviceBuf<double> df;
  hipError_t e = phase_counts(h, nbins, vmin, vmax, d);
  if (e == hipSuccess) e = alloc(df, ((size_t)nb2 + E) * sizeof(double));
  if (e == hipSuccess) e = hipMemcpyAsync(df, feq, (size_t)nb2 * sizeof(double), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    const double dx = h->cfg.L / nbins, dv = (vmax - vmin) / nbins;
    const double norm = h->cfg.n0 / dx / dv / (double)h->cfg.N;                      // objective.py:12, left to right
    hipLaunchKernelGGL(phase_kl_kernel, dim3(E), dim3(BLOCK), 0, h->stream, d, df, df + nb2, nb2, norm, dx * dv);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(kl, df + nb2, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  return hip_tail(h, e, true, "pic_phase_kl");
}

// ---------------------------------------------------------------------------------------------
// Rollout recorder (include/picstep.h: pic_record_*; hooks: advance, pic_step_stage)
// ---------------------------------------------------------------------------------------------
int pic_record_start(pic_handle* h, const pic_record_config* c) {
  if (!h || !c) return fail(h, PIC_EINVAL, "pic_record_start: null argument");
  if (h->rec.on) return fail(h, PIC_ESTATE, "pic_record_start: already recording (pic_record_stop first)");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, "pic_record_start: a staged step is in progress (finish its pic_step_stage calls)");
  const int Ng = h->cfg.Ng;
  const bool phase = c->phase_x_bins > 0 || c->phase_v_bins > 0;
  if (c->stride < 1 || c->n_modes < 0 || c->n_modes > Ng / 2 + 1 || c->x_bins < 0 || c->x_bins > 4096 || c->v_bins < 0 ||
      c->v_bins > 4096 || (phase && (c->phase_x_bins < 1 || c->phase_x_bins > 4096 || c->phase_v_bins < 1 || c->phase_v_bins > 4096)) ||
      !(std::isfinite(c->vmin) && std::isfinite(c->vmax) && c->vmax > c->vmin) || !(c->phase_dx >= 0) || !(c->phase_dv >= 0) ||
      (c->feq && !phase) || c->capacity < 1)
    return fail(h, PIC_EINVAL, "pic_record_start: need stride >= 1, 0 <= n_modes <= Ng/2+1, 0 <= x_bins, v_bins <= 4096, phase bins both 0 "
                               "or both in 1..4096, finite vmin < vmax, phase_dx, phase_dv >= 0, feq only with a phase histogram, capacity >= 1");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  Recorder r;
  r.stride = c->stride; r.M = c->n_modes; r.xb = c->x_bins; r.vb = c->v_bins;
  r.px = phase ? c->phase_x_bins : 0; r.pv = phase ? c->phase_v_bins : 0;
  r.vmin = c->vmin; r.vmax = c->vmax;
  r.pdx = c->phase_dx > 0 ? c->phase_dx : (r.px ? h->cfg.L / r.px : 0.0);
  r.pdv = c->phase_dv > 0 ? c->phase_dv : (r.pv ? (r.vmax - r.vmin) / r.pv : 0.0);
  r.cap = c->capacity;
  r.d_stride = 6 + 2 * (long long)r.M;
  r.u_stride = (long long)r.xb + r.vb + 1;
  const int E = h->cfg.num_envs;
  const size_t nb2 = (size_t)r.px * r.pv;
  const size_t dbytes = (size_t)r.cap * E * r.d_stride * sizeof(double), ubytes = (size_t)r.cap * E * r.u_stride * sizeof(unsigned);
  if ((size_t)r.cap > ((size_t)1 << 40) / ((size_t)E * (r.d_stride * 8 + r.u_stride * 4)))
    return fail(h, PIC_ENOMEM, "pic_record_start: capacity does not fit on the device");
  bool ok = alloc(r.d, dbytes) == hipSuccess && alloc(r.u, ubytes) == hipSuccess &&
            (!nb2 || alloc(r.phase, (size_t)E * nb2 * sizeof(unsigned)) == hipSuccess) &&
            (!c->feq || alloc(r.feq, nb2 * sizeof(double)) == hipSuccess);
  if (!ok) {
    hipGetLastError();
    return fail(h, PIC_ENOMEM, "pic_record_start: capacity does not fit on the device");
  }
  hipError_t e = hipMemsetAsync(r.u, 0, ubytes, h->stream);
  if (e == hipSuccess && nb2) e = hipMemsetAsync(r.phase, 0, (size_t)E * nb2 * sizeof(unsigned), h->stream);
  if (e == hipSuccess && c->feq) e = hipMemcpyAsync(r.feq, c->feq, nb2 * sizeof(double), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(h, PIC_EHIP, std::string("pic_record_start: ") + hipGetErrorString(e));
  if (r.M > 1) {
    const int rc = ensure_twiddle(h, r.M - 1);
    if (rc) return rc;
  }
  r.plan = record_plan(h->cfg.N, h->vec, E, r.xb, r.vb, r.px, r.pv);
  r.on = true;
  h->rec = std::move(r);
  return PIC_OK;
}

int pic_record_now(pic_handle* h) {
  if (!h) return PIC_EINVAL;
  if (!h->rec.on) return fail(h, PIC_ESTATE, "pic_record_now: not recording (pic_record_start first)");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_record_now: call pic_reset first");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, "pic_record_now: a staged step is in progress (finish its pic_step_stage calls)");
  if ((int64_t)h->rec.steps.size() >= h->rec.cap) return fail(h, PIC_ENOMEM, "pic_record_now: the recorder is full");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return record_enqueue(h);
}

int pic_record_count(pic_handle* h, int64_t* n) {
  if (!h || !n) return fail(h, PIC_EINVAL, "pic_record_count: null argument");
  *n = h->rec.on ? (int64_t)h->rec.steps.size() : 0;
  return PIC_OK;
}

int pic_record_read(pic_handle* h, int64_t first, int64_t count, pic_record_out* out) {
  if (!h || !out) return fail(h, PIC_EINVAL, "pic_record_read: null argument");
  const Recorder& r = h->rec;
  if (!r.on) return fail(h, PIC_ESTATE, "pic_record_read: not recording (the records of a stopped recorder are gone)");
  if (first < 0 || count < 0 || first + count > (int64_t)r.steps.size())
    return fail(h, PIC_EINVAL, "pic_record_read: records first..first+count-1 are not all held");
  if (count == 0) return PIC_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t E = (size_t)h->cfg.num_envs, n = (size_t)count;
  std::vector<double> d(n * E * r.d_stride);
  std::vector<unsigned> u(n * E * r.u_stride);
  HIPCHK(h, hipMemcpyAsync(d.data(), r.d + (size_t)first * E * r.d_stride, d.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(u.data(), r.u + (size_t)first * E * r.u_stride, u.size() * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double* scal[6] = {out->KE, out->PE, out->PE_reward, out->field_energy, out->entropy, out->kl};
  const size_t M = (size_t)r.M, xb = (size_t)r.xb, vb = (size_t)r.vb;
  for (size_t i = 0; i < n; ++i) {
    if (out->step) out->step[i] = r.steps[(size_t)first + i];
    for (size_t e = 0; e < E; ++e) {
      const double* src = d.data() + (i * E + e) * r.d_stride;
      const unsigned* us = u.data() + (i * E + e) * r.u_stride;
      for (int q = 0; q < 6; ++q)
        if (scal[q]) scal[q][i * E + e] = src[q];
      if (out->re) std::memcpy(out->re + (i * E + e) * M, src + 6, M * sizeof(double));
      if (out->im) std::memcpy(out->im + (i * E + e) * M, src + 6 + M, M * sizeof(double));
      if (out->x_hist) std::memcpy(out->x_hist + (i * E + e) * xb, us, xb * sizeof(unsigned));
      if (out->v_hist) std::memcpy(out->v_hist + (i * E + e) * vb, us + xb, vb * sizeof(unsigned));
      if (out->inside) out->inside[i * E + e] = us[xb + vb];
    }
  }
  return PIC_OK;
}

int pic_record_stop(pic_handle* h) {
  if (!h) return PIC_EINVAL;
  if (!h->rec.on) return PIC_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const hipError_t e = hipStreamSynchronize(h->stream);
  h->rec = Recorder{};
  return hip_tail(h, e, false, "pic_record_stop");
}

int pic_stream_probe(pic_handle* h, int repeats, double* gbytes_per_s) {
  if (!h || !gbytes_per_s || repeats < 1) return fail(h, PIC_EINVAL, "pic_stream_probe: bad argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t pbytes = (size_t)h->cfg.num_envs * h->ld * h->esz;
  DeviceBuf<double2> a, b;
  HIPCHK(h, alloc(a, pbytes));
  if (alloc(b, pbytes) != hipSuccess) return fail(h, PIC_ENOMEM, "pic_stream_probe: hipMalloc");
  hipMemsetAsync(a, 0, pbytes, h->stream);
  hipMemsetAsync(b, 0, pbytes, h->stream);
  const long long n2 = (long long)(pbytes / sizeof(double2));
  long long nb = n2 / ((long long)BLOCK * 31);       // ~31 tiles per lane, like a sweep workgroup
  if (nb < 256) nb = 256;
  const long long chunk2 = (n2 + nb - 1) / nb;
  EventOwner e0 = make_event(), e1 = make_event();
  hipLaunchKernelGGL(stream_probe_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, h->stream, a.get(), b.get(), n2, chunk2, 1.0, 1);
  hipEventRecord(e0, h->stream);
  for (int r = 0; r < repeats; ++r)
    hipLaunchKernelGGL(stream_probe_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, h->stream, a.get(), b.get(), n2, chunk2, 1.0, r & 1);
  hipEventRecord(e1, h->stream);
  hipError_t e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e != hipSuccess) return fail(h, PIC_EHIP, std::string("pic_stream_probe: ") + hipGetErrorString(e));
  *gbytes_per_s = 4.0 * (double)pbytes * repeats / (ms * 1e-3) / 1e9;
  return PIC_OK;
}

int pic_profile(pic_handle* h, int enable) {
  if (!h) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  prof_drain(h);
  h->prof = enable != 0;
  if (enable) {
    prof_reserve(h, 1024);
    std::memset(h->ms_sum, 0, sizeof(h->ms_sum));
    std::memset(h->launches, 0, sizeof(h->launches));
  }
  return PIC_OK;
}

int pic_profile_read(pic_handle* h, double* ms_sum, int64_t* launches) {
  if (!h) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  prof_drain(h);
  for (int i = 0; i < 8; ++i) {
    if (ms_sum) ms_sum[i] = h->ms_sum[i];
    if (launches) launches[i] = h->launches[i];
  }
  return PIC_OK;
}

int pic_bad_count(pic_handle* h, int64_t* count) {
  if (!h || !count) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  unsigned long long c = 0;
  HIPCHK(h, hipMemcpyAsync(&c, h->bad, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *count = (int64_t)c;
  return PIC_OK;
}

}  // extern "C"