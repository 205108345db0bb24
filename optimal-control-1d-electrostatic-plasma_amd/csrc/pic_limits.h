// pic_limits.h -- the launch constants and sweep stages that the kernels and the host's pure planners (host_plan.h, host_schedule.h)
// share.  No HIP in here: the planners compile with a plain host compiler.  The kernels' static_asserts tie their static __shared__ arrays to the two LDS figures.
#pragma once
#include <cstddef>

constexpr int kMaxFeedbackModes = 16;
constexpr int BLOCK = 512;          // sweep workgroup: 8 waves of 64 (512 beat 256 by 2.7 % and 128 by 11 % at config 2)
constexpr int WAVES = BLOCK / 64;
constexpr size_t kSweepStaticLds = (2 * WAVES + 2) * sizeof(double);     // sweep_kernel's static __shared__ arrays
constexpr size_t kResidentStaticLds = (4 * 8 + 4 + 2 * kMaxFeedbackModes) * sizeof(double);   // resident_kernel's static __shared__ arrays (NW = 8)
// a workgroup may use 64 KB of LDS: the dynamic part the planner sizes plus the kernels' static arrays
constexpr size_t kLdsLimit = 64 * 1024;

// what one launch of sweep_kernel does (its STAGE template parameter); stage_traits below says what each of them is
enum Stage : int { ST_A = 0, ST_B = 1, ST_C = 2, ST_D = 3, ST_REFRESH = 4, ST_PROBE = 5, ST_B2 = 6, ST_D2 = 7, ST_SE = 8, ST_FE = 9, ST_VK = 10,
                   ST_VM = 11, ST_C_RO = 12, ST_D_RC = 13, ST_D2_RC = 14, ST_B2_RO = 15, ST_C_RB = 16, ST_D2_RO = 17, ST_B2_RD = 18 };
constexpr int kStages = ST_B2_RD + 1;
// The arithmetic of a stage.  AR_A .. AR_D are sweeps A .. D of a Yoshida-4 step under the numbers of ST_A .. ST_D: such a sweep's profile
// kind and, for B .. D, the index of the sub-stage's kick in the coefficients d[].  AR_SCHEME: push_scheme, which tells its four stages apart.
enum Arith : int { AR_NONE = -1, AR_A = 0, AR_B = 1, AR_C = 2, AR_D = 3, AR_REFRESH = 4, AR_PROBE = 5, AR_SCHEME = 6 };
// what goes into the second LDS mesh (flushed to SweepIO::acc_out2): nothing, the positions the sweep reads, the next step's q1
enum Mesh2 : int { M2_NONE = 0, M2_INPUT = 1, M2_NEXT_Q1 = 2 };
struct StageTraits {
  Arith arith, rederives;   // the arithmetic it runs itself; the sub-stage it runs in front of that, from its input and the tile in SweepIO::e2
  bool stores, first;       // it stores particles; it deposits into the first LDS mesh (flushed to SweepIO::acc_out)
  Mesh2 second;
};
constexpr StageTraits stage_traits(int stage) {
  switch (stage) {
    //                       arith       rederives stores first  second
    case ST_A:       return {AR_A,       AR_NONE,  false, true,  M2_NONE};     // drift(c) from x,v ; deposit ; nothing stored
    case ST_B:       return {AR_B,       AR_NONE,  true,  true,  M2_NONE};     // recompute q1 = x + (c_prev v) dt ; gather ; kick ; drift ; deposit ; store
    case ST_C:       return {AR_C,       AR_NONE,  true,  true,  M2_NONE};     // gather ; kick ; drift ; deposit ; store
    case ST_D:       return {AR_D,       AR_NONE,  true,  true,  M2_NEXT_Q1};  // as C, then wrap, KE ; store wrapped x ; deposit the next step's q1 as well
    case ST_REFRESH: return {AR_REFRESH, AR_NONE,  true,  true,  M2_NEXT_Q1};  // wrap x ; deposit ; KE ; store wrapped x ; deposit the next step's q1   (pic.py:93-112 on reset)
    case ST_PROBE:   return {AR_PROBE,   AR_NONE,  false, true,  M2_NONE};     // deposit positions of a scratch array, nothing stored             (util.py:73-116 callers)
    // Inside a multi-step call (round 4): the post-step deposit of the final positions x' -- density, E_mesh, phi, PE of the state after
    // a step, which nothing of the next step's dynamics reads -- moves from sweep D, the one sweep bound by VALU issue, into the next
    // step's sweep B, which is bound by memory and reads x' anyway.  Same positions, same cells and weights, same integer sums.
    case ST_B2:      return {AR_B,       AR_NONE,  true,  true,  M2_INPUT};    // as B, and deposits its INPUT positions (the previous step's x') into the second mesh
    case ST_D2:      return {AR_D,       AR_NONE,  true,  false, M2_NEXT_Q1};  // as D without the deposit of x' (wrap, KE, store, the next step's q1 deposit)
    // The one-evaluation schemes and Stormer-Verlet (pic_set_integrator).  Their steps start from the deposit of the
    // stored, wrapped x itself (no first drift), which the step before made as its post-step deposit: one row serves both.
    case ST_SE:      return {AR_SCHEME,  AR_NONE,  true,  true,  M2_NONE};     // symplectic Euler: gather at x ; kick(d) ; drift(c) ; wrap ; deposit x' ; KE ; store
    case ST_FE:      return {AR_SCHEME,  AR_NONE,  true,  true,  M2_NONE};     // forward Euler: gather at x ; drift(c) with the OLD p ; kick(d) ; wrap ; deposit x' ; KE ; store
    case ST_VK:      return {AR_SCHEME,  AR_NONE,  true,  false, M2_NONE};     // Verlet's closing half-kick: gather at q ; kick(d) ; wrap ; KE ; store (no deposit: the input row is x''s)
    case ST_VM:      return {AR_SCHEME,  AR_NONE,  true,  true,  M2_NONE};     // Verlet, merged: as VK, then the next step's half-kick (same field) ; drift(c) ; deposit ; store
    // A whole step inside one call on a state too large for the Infinity Cache (pic_create: readonly_c): sweep C stores nothing and
    // sweep D re-derives C's output from C's input, which is still in memory -- 80 bytes per float64 particle-step instead of 96.
    // The re-derivation is C's own arithmetic on the same operands (push_one: substage), so every bit is the same.
    case ST_C_RO:    return {AR_C,       AR_NONE,  false, true,  M2_NONE};     // as C without the particle stores; workgroup 0 of each environment stores its field tile (SweepIO::e2)
    case ST_D_RC:    return {AR_D,       AR_C,     true,  true,  M2_NEXT_Q1};  // C's sub-stage again from C's input and ST_C_RO's field tile, then as D
    case ST_D2_RC:   return {AR_D,       AR_C,     true,  false, M2_NEXT_Q1};  // ... then as D2
    // Inside such a call every second step (host_schedule.h: a Y step) stores its particles once, in sweep C, and the step behind it
    // opens with a sweep B that re-derives sweep D: three storing sweeps per pair of steps instead of four, 72 bytes per float64
    // particle-step instead of 80.  Each storing sweep re-derives one sub-stage, on the same operands: every bit is the same.
    case ST_B2_RO:   return {AR_B,       AR_NONE,  false, true,  M2_INPUT};    // as B2 without the particle stores; workgroup 0 of each environment stores its field tile (SweepIO::e2)
    case ST_C_RB:    return {AR_C,       AR_B,     true,  true,  M2_NONE};     // B's drift and sub-stage again from B2_RO's input and field tile, then as C (stores)
    case ST_D2_RO:   return {AR_D,       AR_NONE,  false, false, M2_NEXT_Q1};  // as D2 without the particle stores; workgroup 0 of each environment stores its field tile
    case ST_B2_RD:   return {AR_B,       AR_D,     true,  true,  M2_INPUT};    // D's sub-stage and wrap again from D2_RO's input and field tile, then as B2 (stores)
  }
  return {AR_PROBE, AR_NONE, false, true, M2_NONE};      // (no such stage: as ST_PROBE, which touches no state)
}

// What follows from a row: sweep_kernel, push_one, the launch (picstep.hip) and the step schedule (host_schedule.h) ask these.
constexpr bool gathers(StageTraits t) { return (t.arith >= AR_B && t.arith <= AR_D) || t.arith == AR_SCHEME; }   // solves a field in its prologue
constexpr bool reads_v(StageTraits t) { return t.arith != AR_PROBE; }
constexpr bool pushes(StageTraits t) { return t.arith != AR_REFRESH && t.arith != AR_PROBE; }   // a push sweep: it takes a direction
constexpr bool reads_tile(StageTraits t) { return t.rederives != AR_NONE; }                     // ... and needs LDS for a second field tile
constexpr bool leaves_tile(StageTraits t) { return gathers(t) && !t.stores; }                   // the launch behind it re-derives its output
constexpr bool wrap_only(StageTraits t) { return t.arith == AR_D && !t.first; }                 // the D2 kinds end with the wrap, not locate and deposit
constexpr bool ends_step(StageTraits t) { return t.second == M2_NEXT_Q1 || t.arith == AR_SCHEME; }      // sums p^2 per workgroup
constexpr bool carries_solve(StageTraits t) { return t.arith == AR_C; }                         // may carry a riding post-step solve in an extra workgroup
constexpr int profile_kind(StageTraits t) { return t.arith <= AR_D ? (int)t.arith : t.arith == AR_SCHEME ? 7 : 5; }   // (picstep.h: pic_profile_read)
// the kick of the sub-stage a sweep re-derives (its drift is Launch::c_prev), from Yoshida-4's d[]
constexpr double kick_again(StageTraits t, const double* d) { return reads_tile(t) ? d[t.rederives] : 0.0; }

// What sweep_kernel relies on.  One tile buffer: a sweep that left and read a tile would have to read the one before it ahead of storing its own.
// What is re-derived is stored then.  A second mesh exactly where there is something to put there: the q1 behind the end of a Yoshida-4 step, a sweep B's input.
constexpr bool stage_traits_hold() {
  for (int s = 0; s < kStages; ++s) {
    const StageTraits t = stage_traits(s);
    if ((leaves_tile(t) && reads_tile(t)) || (reads_tile(t) && !t.stores) || (t.second == M2_INPUT && t.arith != AR_B) ||
        (t.second == M2_NEXT_Q1) != (t.arith == AR_D || t.arith == AR_REFRESH)) return false;
  }
  return true;
}
static_assert(stage_traits_hold(), "stage_traits: a row contradicts what sweep_kernel relies on");
