// host_schedule.h -- the step schedule of the streaming sweeps (DESIGN.md 4 "Step schedule", 7b): which sweep runs next, which
// ring rows it reads, fills, carries and clears, which of the two field buffers holds a step's field, and whose post-step solve
// rides with which sweep C.  No HIP and no handle in here: the functions below only decide.  Each hands its launches, in launch
// order, to a functor as plain descriptors of slots and roles; picstep.hip's run_launch turns one into kernel arguments and a
// launch.  tests/schedule_driver.cpp is this header as a stand-alone program, and tests/test_schedule_cpu.py holds it to the
// ring's invariants over every short order of calls.
#pragma once

#include "picstep.h"

#include "pic_limits.h"

constexpr int RING = 8;             // accumulator rows in rotation (row RING of the allocation is the probes' own)
constexpr int ST_SOLVE = -1;        // Launch::stage of a field solve launched on its own

// force evaluations per step of an integrator (pic_get_integrator, pic_step_stage)
inline int evals_per_step(int scheme) { return scheme == PIC_YOSHIDA4 ? 3 : (scheme == PIC_VERLET ? 2 : 1); }

// The accumulator ring's bookkeeping.  A row is clean (zero), dirty (retired: every kernel reading it has been enqueued, any later
// sweep may clear it) or held by whoever took it.
struct Ring {
  int clean[RING], dirty[RING];     // a stack and a queue
  int nclean = RING, ndirty = 0;
  Ring() { for (int s = 0; s < RING; ++s) clean[s] = s; }

  // a row for the deposit of the launch about to be made.  *unclean: the guard was needed -- no clean row was left, the row
  // comes from the dirty list and the caller has to clear it first.  The step schedule never gets there: every sweep clears two
  // retired rows, and tests/test_schedule_cpu.py asserts it for every order of calls to depth 4 and for long random ones.
  int take(bool* unclean) {
    if (nclean > 0) return clean[--nclean];
    *unclean = true;
    return pop_retired();
  }
  // the last kernel reading `slot` has been enqueued
  void retire(int slot) {
    if (slot >= 0) dirty[ndirty++] = slot;
  }
  // the oldest retired row, for the sweep about to be launched to clear; -1: none
  int pop_retired() {
    if (ndirty == 0) return -1;
    const int s = dirty[0];
    for (int k = 1; k < ndirty; ++k) dirty[k - 1] = dirty[k];
    --ndirty;
    return s;
  }
  // that sweep has been enqueued: the row is zero for every LATER launch of the stream
  void cleared(int slot) {
    if (slot >= 0) clean[nclean++] = slot;
  }
};

// What the streaming schedule remembers between two calls (embedded in the handle)
struct Schedule {
  Ring ring;
  int q_slot = -1;                // row holding the deposit the NEXT step starts from: Yoshida-4's q1 (sweep A is skipped while >= 0),
                                  // the other integrators' x
  int stage_slot = -1;            // pic_step_stage: row the next stage's field comes from
  int mid_stage = 0;              // pic_step_stage: force evaluations of the current step already done (0 = between steps)
  int sweep_parity = 0;           // direction of the last push sweep
  int ext_turn = 0;               // which of the two field buffers holds the field of the step being launched

  // the cached deposits belong to particles that are about to change under other hands (the resident kernel)
  void drop_rows() {
    ring.retire(q_slot);
    ring.retire(stage_slot);
    q_slot = stage_slot = -1;
  }
};

enum CtlRole : int { CTL_NONE = 0, CTL_OWN = 1, CTL_SHARED = 2 };     // no external field / the call's own control of Launch::step /
                                                                     // the field of that step, built once per environment
enum ExtRole : int { EXT_NONE = 0, EXT_THIS = 1, EXT_NEXT = 2 };     // the buffer of this step's field (Launch::turn) / the other one

// One launch: a sweep over all environments, or a field solve of its own.  Slots and roles, never device pointers.
struct Launch {
  int stage = ST_SOLVE;                      // a Stage, or ST_SOLVE
  double c_prev = 0, d_prev = 0, c_cur = 0, d_cur = 0;   // a sweep's stage coefficients (d_prev: the kick of the sub-stage it re-derives, or 0)
  int in = -1;                               // ring row the gather field is solved from; a solve: the row it solves
  int fill[2] = {-1, -1};                    // rows receiving the first / second deposit (RING: the probes' row)
  int unclean = 0;                           // bit k: fill[k] came from Ring::take's guard and must be cleared before the launch
  int post = -1;                             // sweep C: row whose post-step solve rides in one extra workgroup per environment
  int clear[2] = {-1, -1};                   // retired rows this sweep clears
  int reverse = 0;                           // direction of a push sweep
  int ctl = CTL_NONE;                        // the control its force evaluation reads
  int ext_out = EXT_NONE;                    // the buffer it writes a step's field into
  int turn = 0;                              // which buffer is "this step's" (Schedule::ext_turn at the launch)
  bool hand_on = false;                      // sweep D builds the next step's field, from the action of step + 1
  int step = 0;                              // index within the call of the step it belongs to: its per-step control, its history row
  int post_step = -1;                        // ... of the step the riding solve records for
  bool retire = false;                       // a solve: its row retires behind it
  bool feedback = false;                     // a solve: it also computes the feedback law's action of step + 1
};

// The shape of a call of whole steps
struct CallShape {
  int scheme = PIC_YOSHIDA4;
  const double* cs = nullptr;            // Yoshida-4's coefficients (LaunchPlan::cs, ds)
  const double* ds = nullptr;
  bool light_inner_steps = false;        // LaunchPlan: inner steps end with sweep D2
  bool readonly_c = false;               // whole steps run sweeps C_RO and D_RC / D2_RC
  bool alternate_stores = false;         // ... and every second inner step of a call stores its particles once (alternates below)
  bool feedback = false;                 // the on-device feedback law drives the field
  bool action = false;                   // the control is an actuator's action (not a field, or nothing)
  bool per_step_field = false;           // a new field / a new action with every step (else held for the call)
  bool per_step_action = false;
};

// What one call keeps between its launches.  It dies with the call; a call ends with all of it at rest (plan_call returns it
// for the CPU test to see).
struct CallLocals {
  int post = -1;                  // ring row whose post-step solve rides with the next sweep C
  int post_step = -1;             // the step that solve records its energies for
  bool refresh_pending = false;   // the last sweep was a D2: the next sweep B deposits the positions it reads
  bool open = false;              // Verlet: a merged sweep has already made this step's opening half-kick and drift
};

namespace schedule_detail {

inline int take(Schedule& S, Launch& l, int k) {
  bool unclean = false;
  l.fill[k] = S.ring.take(&unclean);
  if (unclean) l.unclean |= 1 << k;
  return l.fill[k];
}

// the sweep also clears up to two retired ring rows for later use
template <typename F>
void emit_sweep(Schedule& S, Launch& l, F& emit) {
  l.reverse = pushes(stage_traits(l.stage)) ? (S.sweep_parity ^= 1) : 0;
  l.turn = S.ext_turn;
  for (int k = 0; k < 2; ++k) l.clear[k] = S.ring.pop_retired();
  emit(static_cast<const Launch&>(l));
  for (int k = 0; k < 2; ++k) S.ring.cleared(l.clear[k]);
}

// the post-step refresh (pic.py:145-146, no external field: pic.py:114-117) from the deposit in `row`; retire = false (the other
// integrators): the row stays, as the deposit the next step's force is solved from
template <typename F>
void emit_solve(Schedule& S, int row, bool retire, int step, bool feedback, F& emit) {
  Launch l;
  l.in = row; l.retire = retire; l.step = step; l.feedback = feedback; l.turn = S.ext_turn;
  emit(static_cast<const Launch&>(l));
  if (retire) S.ring.retire(row);
}

// one step of a call, as the stages below see it
struct StepShape {
  int step = 0;
  bool another = false;        // a further step of the call follows and takes over this step's post-step solve
  bool field_ready = false;    // the previous step's sweep D has built this step's field
  bool hand_on = false;        // this step's sweep D builds the next one's
  bool feedback = false;       // this step's solve computes the next action
  bool alternate = false;      // the call alternates its stores (alternates below): its inner steps end with a D2 flavour
  bool lean = false;           // ... and this is a Y step: sweeps B2_RO, C_RB, D2_RO
  bool after_lean = false;     // ... or the step behind one: its sweep B is B2_RD
};

// Does a call of nsteps whole steps store its particles in every other sweep?  Only where the read-only sweep C is in force, in a
// call of two or more Yoshida-4 steps; not under the feedback law, which needs each step's field before the next sweep B.
inline bool alternates(const CallShape& p, int nsteps) {
  return p.alternate_stores && p.readonly_c && p.scheme == PIC_YOSHIDA4 && !p.feedback && nsteps >= 2;
}
// Inside such a call the steps are of two kinds.  X is the step of every other call: B or B2 (stores), C_RO, D2_RC or D_RC (stores).
// Y stores once: B2_RO, C_RB (re-derives B, stores), D2_RO; the X step behind it opens with B2_RD, which re-derives D.  A call
// begins with an X step (it reads stored state) and ends with one (state and fields are in memory when it returns), and no two Y
// steps follow each other: step i of K is Y exactly when i >= 1 and K - 1 - i is odd.  Storing sweeps: 2 K - floor((K - 1) / 2).
inline bool lean_step(int i, int nsteps) { return i >= 1 && ((nsteps - 1 - i) & 1) != 0; }

// The sweeps of one Yoshida-4 step, stages from..upto (1 = sweep B, 2 = C, 3 = D; 1..3: a whole step inside a call).
// another (the steps of one call but the last): on a large state (light_inner_steps) the step ends with sweep D2, which leaves
// the deposit of its final positions to the next step's sweep B2; either way its post-step solve is not launched: that step's
// sweep C carries it in one extra workgroup per environment (its results -- n, E_mesh, phi, the energies -- are read by nothing
// inside the call; the last step ends with the full sweep D and a solve launch of its own as ever).  Every refresh is made, from
// the same integer sums.
template <typename F>
void yoshida_stages(Schedule& S, const CallShape& p, int from, int upto, const StepShape& st, CallLocals& L, F& emit) {
  const double* c = p.cs;
  const double* d = p.ds;
  const bool whole = from == 1 && upto == 3;
  // A whole step under actuator coefficients builds the actuator's field once per environment, not in every workgroup of every
  // sweep (pic_sweep.h: SweepIO::ext_out).  The handle's two field buffers -- idle in such a call: they stage host fields -- take
  // turns: this step's is written by sweep B of a call's first step (which builds it in every workgroup: it cannot wait for
  // anyone) or by the previous step's sweep D (field_ready); sweep D writes the next step's from the next action into the other
  // one.  Same doubles, same sums: config 3 as specified pays 0.5 % for its control instead of 2.6 %.
  const bool share = whole && (p.action || p.feedback);
  const int later = share ? CTL_SHARED : CTL_OWN;
  // A whole step runs sweep C without its stores where the handle chose it (readonly_c): sweep D re-derives them.  A staged step
  // keeps them, since its caller may read the particles between the stages.
  const bool ro = whole && p.readonly_c;
  for (int stage = from; stage <= upto; ++stage) {
    Launch l;
    l.step = st.step;
    if (stage == 1) {
      if (S.q_slot < 0) {          // particles were loaded without a refresh: deposit q1 = x + (c1 v) dt now
        Launch a;
        a.stage = ST_A; a.c_cur = c[0]; a.step = st.step;
        S.q_slot = take(S, a, 0);
        emit_sweep(S, a, emit);
      }
      l.stage = !L.refresh_pending ? ST_B : st.lean ? ST_B2_RO : st.after_lean ? ST_B2_RD : ST_B2;
      l.c_prev = l.stage == ST_B2_RD ? c[3] : c[0]; l.c_cur = c[1]; l.d_cur = d[1];     // (B2_RD: the drift of sweep D, which it re-derives)
      l.d_prev = kick_again(stage_traits(l.stage), d);
      l.in = S.q_slot;
      l.ctl = share && st.field_ready ? CTL_SHARED : CTL_OWN;
      l.ext_out = share && !st.field_ready ? EXT_THIS : EXT_NONE;
      const int x1 = take(S, l, 0);
      // the step before ended with sweep D2: this sweep B deposits the positions it reads (that step's x') into a second row, and
      // sweep C carries the post-step solve of that step from it
      if (L.refresh_pending) L.post = take(S, l, 1);
      L.refresh_pending = false;
      emit_sweep(S, l, emit);
      S.ring.retire(S.q_slot);
      S.q_slot = -1;
      S.stage_slot = x1;
    } else if (stage == 2) {
      l.stage = st.lean ? ST_C_RB : ro ? ST_C_RO : ST_C;
      l.c_prev = st.lean ? c[1] : 0.0; l.c_cur = c[2]; l.d_cur = d[2];                  // (C_RB: the drift of sweep B, which it re-derives)
      l.d_prev = kick_again(stage_traits(l.stage), d);
      l.in = S.stage_slot;
      l.ctl = later;
      l.post = L.post;
      l.post_step = L.post >= 0 ? L.post_step : -1;
      const int x2 = take(S, l, 0);
      emit_sweep(S, l, emit);
      S.ring.retire(L.post);
      L.post = -1;
      S.ring.retire(S.stage_slot);
      S.stage_slot = x2;
    } else {
      l.c_prev = ro && !st.lean ? c[2] : 0.0; l.c_cur = c[3]; l.d_cur = d[3];
      l.in = S.stage_slot;
      l.ctl = later;
      l.hand_on = share && st.hand_on;
      l.ext_out = l.hand_on ? EXT_NEXT : EXT_NONE;
      if (st.another && (p.light_inner_steps || st.alternate)) {
        // an inner step of a call: nothing can see its post-step fields before the next step has started, so the deposit they come
        // from is left to that step's sweep B2 (sweep D is the one sweep bound by VALU issue: 336 -> 321 us at config 2, B 320 -> 322)
        l.stage = st.lean ? ST_D2_RO : ro ? ST_D2_RC : ST_D2; l.d_prev = kick_again(stage_traits(l.stage), d);
        const int qn = take(S, l, 1);
        emit_sweep(S, l, emit);
        L.refresh_pending = true;
        L.post_step = st.step;
        S.q_slot = qn;
      } else {
        l.stage = ro ? ST_D_RC : ST_D; l.d_prev = kick_again(stage_traits(l.stage), d);
        const int f = take(S, l, 0), qn = take(S, l, 1);
        emit_sweep(S, l, emit);
        // (a small state's inner step: the full sweep D, its solve still not a launch -- it rides with the next step's sweep C)
        if (st.another) { L.post = f; L.post_step = st.step; }
        else emit_solve(S, f, true, st.step, st.feedback, emit);
        S.q_slot = qn;
      }
      if (l.hand_on) S.ext_turn ^= 1;
      S.ring.retire(S.stage_slot);
      S.stage_slot = -1;
    }
  }
}

// ---- the other integrators (pic_set_integrator) ----------------------------------------------------------------------
// Between steps q_slot holds the deposit of the stored, wrapped x: the post-step deposit of the step before, which is also the
// field of the next step's (first) force evaluation -- one row, no first drift to deposit.  Where it is missing (particles loaded
// without a refresh, or a Yoshida-4 q1 dropped by a change of scheme) a probe sweep deposits x.
template <typename F>
void scheme_first_deposit(Schedule& S, int step, F& emit) {
  if (S.q_slot >= 0) return;
  Launch l;
  l.stage = ST_PROBE; l.step = step;
  S.q_slot = take(S, l, 0);
  emit_sweep(S, l, emit);
}

// One step's sweeps, or its stage `only` (1..2 of Verlet) for pic_step_stage.  merge (Verlet, a further step follows with the
// same external field): the closing half-kick of this step and the opening half-kick and drift of the next one are ONE sweep
// (ST_VM), two additions in the order separate sweeps make them; L.open tells the next step that its opening sweep is done.
template <typename F>
void scheme_step(Schedule& S, int scheme, int only, bool merge, const StepShape& st, CallLocals& L, F& emit) {
  Launch l;
  l.step = st.step; l.ctl = CTL_OWN; l.in = S.q_slot;
  if (scheme != PIC_VERLET) {
    scheme_first_deposit(S, st.step, emit);
    l.stage = scheme == PIC_SYMPLECTIC_EULER ? ST_SE : ST_FE;      // integration.py:50-51 (c = d = 1) / :8-10
    l.c_cur = 1.0; l.d_cur = 1.0; l.in = S.q_slot;
    const int f = take(S, l, 0);
    emit_sweep(S, l, emit);
    S.ring.retire(S.q_slot);
    emit_solve(S, f, false, st.step, st.feedback, emit);
    S.q_slot = f;
    return;
  }
  if (only != 2 && !L.open) {                                  // step(c = 1, d = 0.5): kick, drift, deposit of q' (a sweep C)
    scheme_first_deposit(S, st.step, emit);
    Launch o = l;
    o.stage = ST_C; o.c_cur = 1.0; o.d_cur = 0.5; o.in = S.q_slot;
    const int r = take(S, o, 0);
    emit_sweep(S, o, emit);
    S.ring.retire(S.q_slot);
    S.q_slot = r;
  }
  if (only == 1) return;
  l.in = S.q_slot; l.d_cur = 0.5;
  if (merge) {                                                 // step(c = 0, d = 0.5), then the next step's step(c = 1, d = 0.5)
    l.stage = ST_VM; l.c_cur = 1.0;
    const int r = take(S, l, 0);
    emit_sweep(S, l, emit);
    emit_solve(S, S.q_slot, true, st.step, st.feedback, emit);   // this step's refresh: KE from the merged sweep, n and E from x''s deposit
    S.q_slot = r;
    L.open = true;
  } else {                                                     // step(c = 0, d = 0.5): the closing half-kick alone
    l.stage = ST_VK;
    emit_sweep(S, l, emit);
    emit_solve(S, S.q_slot, false, st.step, st.feedback, emit);
    L.open = false;
  }
}

}  // namespace schedule_detail

// pic_invalidate and every reload: no cached deposit outlives the particles it was made from; an open staged step is abandoned
inline void plan_drop(Schedule& S) {
  S.drop_rows();
  S.mid_stage = 0;
}

// the fields of the particles as they stand (pic_reset, pic_refresh): one sweep, one solve
template <typename F>
void plan_refresh(Schedule& S, int scheme, F&& emit) {
  using namespace schedule_detail;
  plan_drop(S);
  Launch l;
  l.stage = ST_REFRESH;
  const int f = take(S, l, 0), qn = take(S, l, 1);
  emit_sweep(S, l, emit);
  if (scheme == PIC_YOSHIDA4) {
    emit_solve(S, f, true, 0, false, emit);
    S.q_slot = qn;   // ST_REFRESH also deposited the next step's q1
  } else {
    emit_solve(S, f, false, 0, false, emit);
    S.ring.retire(qn);
    S.q_slot = f;    // the other integrators start from the deposit of x itself
  }
}

// a field probe's deposit into the probes' own row: no step state is touched, but like every sweep it clears two retired rows
template <typename F>
void plan_probe(Schedule& S, F&& emit) {
  Launch l;
  l.stage = ST_PROBE;
  l.fill[0] = RING;
  schedule_detail::emit_sweep(S, l, emit);
}

// pic_step_stage: force evaluation `stage` (1..S of the scheme, the caller has checked the order) under the call's own control
template <typename F>
void plan_stage(Schedule& S, const CallShape& p, int stage, F&& emit) {
  using namespace schedule_detail;
  CallLocals L;
  const int evals = evals_per_step(p.scheme);
  if (p.scheme == PIC_YOSHIDA4) yoshida_stages(S, p, stage, stage, StepShape{}, L, emit);
  else scheme_step(S, p.scheme, evals == 1 ? 0 : stage, false, StepShape{}, L, emit);
  S.mid_stage = stage == evals ? 0 : stage;
}

// nsteps whole steps in one call.  Yoshida-4: the actuator's field of step s is built by sweep B of step 0, after that by the
// previous step's sweep D -- or, under a held action, still the one step 0 left; the feedback law's action exists only after the
// post-step solve (a launch of its own that also computes the next action, nothing rides): every step builds.  Verlet merges
// where the two half-kicks of a merged sweep see one external field: held for the call.  A new field every step, or the feedback
// law's, runs two sweeps per step.
template <typename F>
CallLocals plan_call(Schedule& S, const CallShape& p, int nsteps, F&& emit) {
  using namespace schedule_detail;
  CallLocals L;
  const bool rollout = !p.feedback && p.action;
  const bool held = !p.feedback && !p.per_step_field && !p.per_step_action;
  const bool alt = alternates(p, nsteps);
  for (int s = 0; s < nsteps; ++s) {
    const bool last = s + 1 == nsteps;
    StepShape st;
    st.step = s;
    st.feedback = p.feedback && !last;
    if (p.scheme == PIC_YOSHIDA4) {
      st.another = !last && !p.feedback;
      st.field_ready = rollout && s > 0;
      st.hand_on = rollout && p.per_step_action && !last;
      st.alternate = alt;
      st.lean = alt && lean_step(s, nsteps);
      st.after_lean = alt && s > 0 && lean_step(s - 1, nsteps);
      yoshida_stages(S, p, 1, 3, st, L, emit);
    } else {
      scheme_step(S, p.scheme, 0, held && !last, st, L, emit);
    }
  }
  return L;
}
