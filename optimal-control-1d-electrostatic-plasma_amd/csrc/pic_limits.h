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

// what one launch of sweep_kernel does (its STAGE template parameter)
enum Stage : int {
  ST_A = 0,        // drift(c) from x,v ; deposit ; nothing stored
  ST_B = 1,        // recompute q1 = x + (c_prev v) dt ; gather ; kick ; drift ; deposit ; store
  ST_C = 2,        // gather ; kick ; drift ; deposit ; store
  ST_D = 3,        // as C, then wrap, KE ; store wrapped x ; deposit the next step's q1 as well
  ST_REFRESH = 4,  // wrap x ; deposit ; KE ; store wrapped x ; deposit the next step's q1   (pic.py:93-112 on reset)
  ST_PROBE = 5,    // deposit positions of a scratch array, nothing stored             (util.py:73-116 callers)
  // Inside a multi-step call (round 4): the post-step deposit of the final positions x' -- density, E_mesh, phi, PE of the state after
  // a step, which nothing of the next step's dynamics reads -- moves from sweep D, the one sweep bound by VALU issue, into the next
  // step's sweep B, which is bound by memory and reads x' anyway.  Same positions, same cells and weights, same integer sums.
  ST_B2 = 6,       // as B, and deposits its INPUT positions (the previous step's x') into the second mesh
  ST_D2 = 7,       // as D without the deposit of x' (wrap, KE, store, the next step's q1 deposit)
  // The one-evaluation schemes and Stormer-Verlet (pic_set_integrator).  Their steps start from the deposit of the
  // stored, wrapped x itself (no first drift), which the step before made as its post-step deposit: one row serves both.
  ST_SE = 8,       // symplectic Euler: gather at x ; kick(d) ; drift(c) ; wrap ; deposit x' ; KE ; store
  ST_FE = 9,       // forward Euler: gather at x ; drift(c) with the OLD p ; kick(d) ; wrap ; deposit x' ; KE ; store
  ST_VK = 10,      // Verlet's closing half-kick: gather at q ; kick(d) ; wrap ; KE ; store (no deposit: the input row is x''s)
  ST_VM = 11,      // Verlet, merged: as VK, then the next step's half-kick (same field) ; drift(c) ; deposit ; store
  // A whole step inside one call on a state too large for the Infinity Cache (pic_create: readonly_c): sweep C stores nothing and
  // sweep D re-derives C's output from C's input, which is still in memory -- 80 bytes per float64 particle-step instead of 96.
  // The re-derivation is C's own arithmetic on the same operands (push_one: substage), so every bit is the same.
  ST_C_RO = 12,    // as C without the particle stores; workgroup 0 of each environment stores its field tile (SweepIO::e2)
  ST_D_RC = 13,    // C's sub-stage again from C's input and ST_C_RO's field tile, then as D
  ST_D2_RC = 14,   // ... then as D2
  // Inside such a call every second step (host_schedule.h: a Y step) stores its particles once, in sweep C, and the step behind it
  // opens with a sweep B that re-derives sweep D: three storing sweeps per pair of steps instead of four, 72 bytes per float64
  // particle-step instead of 80.  Each storing sweep re-derives one sub-stage, on the same operands: every bit is the same.
  ST_B2_RO = 15,   // as B2 without the particle stores; workgroup 0 of each environment stores its field tile (SweepIO::e2)
  ST_C_RB = 16,    // B's drift and sub-stage again from B2_RO's input and field tile, then as C (stores)
  ST_D2_RO = 17,   // as D2 without the particle stores; workgroup 0 of each environment stores its field tile
  ST_B2_RD = 18    // D's sub-stage and wrap again from D2_RO's input and field tile, then as B2 (stores)
};
