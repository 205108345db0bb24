/*
 * picstep.h -- C ABI of libpicstep.so, the MI355X (gfx950) 1-D electrostatic PIC stepper.
 *
 * The reference (ZINZINBIN/Optimal-Control-1D-Electrostatic-Plasma) has no FFI layer: its
 * boundary is the Python duck type `PIC` (src/env/pic.py:11-223).  Each entry point below names
 * the reference interface it stands in for; the ctypes binding lives in
 * optimal-control-1d-electrostatic-plasma_amd/_abi.py and INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions: every function returns 0 on success or a negative PIC_E* code (text through
 * pic_last_error); no exception crosses the ABI; the library owns all device memory; host
 * buffers are caller-owned and copied.  One handle = one device = one HIP stream; calls on one
 * handle must be serialised by the caller, different handles are independent (one per GPU when
 * environments are sharded).  All entry points except pic_step / pic_reset (device inputs)
 * return after the stream has drained; pic_step is asynchronous -- call pic_sync or any getter.
 *
 * Particle arrays are [num_envs][ld] with ld >= N (ld from pic_device_ptrs); host copies are
 * dense [num_envs][N].  Mesh arrays are dense [num_envs][Ng] float64.
 */
#ifndef PICSTEP_H
#define PICSTEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PICSTEP_ABI_VERSION 5

enum { PIC_F64 = 0, PIC_F32 = 1 };           /* particle dtype (velocities; positions too unless fixed point) */
enum { PIC_POS_FLOAT = 0,                    /* positions stored in the particle dtype                         */
       PIC_POS_FIXED32 = 1 };                 /* positions as 32-bit fixed point, x = u L / 2^32 (float32 particles) */
enum { PIC_ACC_AUTO = 0,                     /* deposit accumulator: library's choice (PACKED for float32 CIC, else FIX64) */
       PIC_ACC_FIX64 = 1,                     /* 64-bit integers, weights rounded to 2^-fg: order-independent sums    */
       PIC_ACC_PACKED = 2,                    /* float32 particles, CIC: (count, sum of w_r) per cell in one word     */
       PIC_ACC_F64 = 3 };                     /* float64 particles: float64 running sums in LDS (ds_add_f64)          */
enum { PIC_CIC = 0, PIC_TSC = 1 };           /* src/env/interpolate.py:4 (CIC), :22 (TSC)     */
enum { PIC_YOSHIDA4 = 0,                     /* time integrator of a step (pic_set_integrator), src/env/integration.py: */
       PIC_SYMPLECTIC_EULER = 1,              /*   symplectic_4th_order (:60, the default), symplectic_euler (:50),     */
       PIC_VERLET = 2,                        /*   verlet (:54), forward_euler (:8)                                     */
       PIC_FORWARD_EULER = 3 };
enum { PIC_PLACE_AUTO = 0,                   /* large states: look for x and v in two different regions of HBM (pic_placement_info) */
       PIC_PLACE_OFF = 1 };                   /* no search: x | v in one allocation                                                 */
enum { PIC_HOST = 0, PIC_DEVICE = 1 };       /* where a caller buffer lives                   */
enum { PIC_PLACED_NONE = 0,                  /* pic_placement.outcome: no search (small state or PIC_PLACE_OFF)                    */
       PIC_PLACED_FOUND = 1,                 /* the pair kept streams >= 10 % faster than the slowest pair seen                    */
       PIC_PLACED_PATIENCE = 2,              /* 42 GiB walked without an improvement: all alike, the best of them kept             */
       PIC_PLACED_TIMEOUT = 3,               /* the leg's 100 ms spent: the best pair seen so far kept; a reset may run another leg */
       PIC_PLACED_MEMORY = 4 };              /* a third of the free memory held (or an allocation failed): the best pair seen kept */

enum {
  PIC_OK = 0,
  PIC_EINVAL = -1,     /* bad argument / unsupported configuration   */
  PIC_EHIP = -2,       /* a HIP runtime call failed                  */
  PIC_ESTATE = -3,     /* call order (e.g. step before reset)        */
  PIC_ENOMEM = -4
};

/* Constructor arguments of PIC (src/env/pic.py:13-27) that matter to the step, plus batching.
 * dt is the value AFTER the CFL clamp of pic.py:71-73 (the host wrapper applies the clamp).
 * gamma is accepted for signature parity only: E_mesh does not depend on it. */
typedef struct pic_config {
  int64_t N;               /* particles per environment                                   */
  int32_t Ng;              /* mesh cells (N_mesh)                                         */
  int32_t num_envs;        /* independent environments batched on this device             */
  double  L;               /* box length                                                  */
  double  n0;              /* mean density                                                */
  double  dt;              /* time step (post-clamp)                                      */
  double  gamma;           /* unused by the scan solver                                   */
  int32_t particle_dtype;  /* PIC_F64 | PIC_F32                                           */
  int32_t accum_dtype;     /* PIC_ACC_*: how a workgroup accumulates its deposit in LDS.  Every choice ends in the
                              same global 64-bit fixed-point accumulators; FIX64 and PACKED are integer sums all
                              the way and make a step bitwise reproducible                        */
  int32_t interpol;        /* PIC_CIC | PIC_TSC                                           */
  int32_t device_id;       /* HIP device ordinal                                          */
  int32_t blocks_per_env;  /* 0 = choose the schedule: environments of up to 8192 particles are stepped RESIDENT (all
                              sub-stages and steps of a pic_step call inside one workgroup and one launch), larger ones
                              by streaming sweeps over a chosen number of workgroups; > 0 = streaming sweeps with this
                              many workgroups per environment; -1 = resident, or EINVAL where it does not apply.
                              Particles and fields do not depend on the choice, bit for bit                       */
  int32_t env_index_base;  /* global index of environment 0 of this handle (0 for a single handle): keys the device
                              sampler, so that a sharded ensemble does not depend on the number of ranks           */
  int32_t position_dtype;  /* PIC_POS_FLOAT | PIC_POS_FIXED32 (needs particle_dtype PIC_F32).  Fixed-point positions
                              are handed over and returned as float32 like any float32 particle array; on the device
                              they are uint32 (pic_device_ptrs' x)                                                  */
  int32_t placement;       /* PIC_PLACE_AUTO | PIC_PLACE_OFF: see pic_placement_info                                */
  int32_t placement_ms;    /* upper bound, in milliseconds, on one leg of the search for an (x, v) placement; 0 = the
                              default (100 ms, or forty steps' worth of the handle if that is more)                  */
} pic_config;

typedef struct pic_handle pic_handle;

/* PIC.__init__ (pic.py:13-61) minus sampling: allocates state for num_envs environments. */
int pic_create(const pic_config* cfg, pic_handle** out);
int pic_destroy(pic_handle* h);

/* PIC.initialize / reinit (pic.py:63-91) after the host has drawn x0, v0 and applied the velocity
 * perturbation: stores the particles and does update_density + update_E_field (pic.py:93-123).
 * x0, v0: [num_envs][N] of the particle dtype, host or device. */
int pic_reset(pic_handle* h, const void* x0, const void* v0, int mem_kind);

/* PIC.reinit with the sample drawn ON THE DEVICE: the distributions of src/env/dist.py (kind 0 =
 * TwoStream :27-102, halves at +v0 / -v0 with spread sigma; kind 1 = BumpOnTail :104-194, int(N/(1+a))
 * bulk particles from N(0,1) followed by the beam from N(v0, sigma) -- the index order high_indx relies
 * on), x uniform on [0, L), v truncated to [-10, 10], then the velocity perturbation
 * v *= 1 + A sin(2 pi n_mode x / L) (pic.py:68) and update_density + update_E_field.  Counter-based
 * Philox generator keyed by (seed, environment): reproducible, but NOT the reference's NumPy stream --
 * the host samplers of the Python layer keep that.  Every velocity before the perturbation lies in
 * [-10, 10] (a particle whose 63 rejection attempts all fall outside draws from the truncated normal).
 * PIC_EINVAL for sigma < 1/sqrt(2 pi): the reference accepts with u < pdf(v), so where the peak of pdf
 * exceeds 1 its density is min(pdf, 1), which this sampler does not reproduce -- use the host samplers. */
int pic_reset_sampled(pic_handle* h, int kind, double a, double v0, double sigma, double A, int n_mode,
                      uint64_t seed);

/* nsteps x PIC.update_state(E_external) (pic.py:131-146): Yoshida-4 push
 * (src/env/integration.py:60-75), final wrap, density/field refresh, KE/PE reductions.
 * E_ext: NULL or [num_envs][Ng] float64 (held constant over the nsteps), host or device.
 * Asynchronous on the handle's stream. */
int pic_step(pic_handle* h, const double* E_ext, int mem_kind, int nsteps);

/* PIC.x / PIC.v / get_state (pic.py:165-167): copies of the particle arrays, dense [num_envs][N]. */
int pic_get_particles(pic_handle* h, void* x, void* v, int mem_kind);
/* Overwrite the particles without touching fields (checkpoint restore); follow with pic_refresh. */
int pic_set_particles(pic_handle* h, const void* x, const void* v, int mem_kind);
/* update_density + update_E_field on the current particles (pic.py:93-123). */
int pic_refresh(pic_handle* h);
/* The caller has written x or v through the device views of pic_device_ptrs (e.g. re-seeded finished
 * environments on the device).  The handle caches the next step's first deposit (taken by the last sweep
 * of the previous step); that cache no longer matches such particles.  pic_invalidate drops it, so that the
 * next pic_step re-deposits from the stored particles (one extra read of x, v); pic_refresh does the same and
 * also recomputes n / E_mesh / phi / energies.  One of the two MUST follow every external write. */
int pic_invalidate(pic_handle* h);

/* Zero-copy device views for torch: any pointer argument may be NULL. ld = leading dimension
 * (elements) of x and v; mesh arrays are dense. Valid until pic_destroy.  The views are writable; a write to
 * x or v must be followed by pic_invalidate or pic_refresh (see there). */
int pic_device_ptrs(pic_handle* h, void** x, void** v, int64_t* ld, double** n, double** E_mesh, double** phi,
                    double** KE, double** PE, double** PE_reward);

/* PIC.n, PIC.E_mesh, PIC.phi_mesh after a step (pic.py:103,116-117). phi is returned in the
 * mean-zero gauge (the reference's gauge is round-off). Host buffers, any may be NULL. */
int pic_get_fields(pic_handle* h, double* n, double* E_mesh, double* phi);

/* Per-environment energies of the current state: KE = 0.5*sum v^2 (src/env/util.py:144),
 * PE = 0.5*sum(E_mesh^2)*dx*N/L (util.py:129-130), PE_reward = 0.5*sum(E_mesh^2)*dx
 * (src/control/objective.py:33, the reward reduction). Host buffers [num_envs], any may be NULL. */
int pic_get_energies(pic_handle* h, double* KE, double* PE, double* PE_reward);

/* PIC.E (pic.py:120): E_mesh gathered at the particles, dense [num_envs][N], particle dtype. */
int pic_gather_E(pic_handle* h, void* E_particles, int mem_kind);

/* PIC.indx_l/indx_r/weight_l/weight_r (pic.py:104-107) of one environment: host buffers [N]
 * (int64 indices, float64 weights), any may be NULL. */
int pic_get_cic(pic_handle* h, int env, int64_t* indx_l, int64_t* indx_r, double* weight_l, double* weight_r);

/* compute_E on arbitrary positions (src/env/util.py:73-116), used by compute_electric_energy
 * (util.py:119-131) and estimate_electric_energy (objective.py:20-35): deposit x -> solve ->
 * E_mesh (+E_ext).  Does not modify the environments' state (probes have their own deposit accumulator and
 * E_ext staging, so they may also run between pic_step_stage calls), pic_bad_count included: a non-finite
 * probe position is deposited at x = 0 and counted nowhere (same for pic_compute_E).  x: [num_envs][N] particle dtype;
 * E_ext: NULL or [num_envs][Ng] host float64; outputs (host, [num_envs][Ng] / [num_envs], any
 * may be NULL): n, E_mesh (with E_ext added), half_sum_E2_dx = 0.5*sum(E_mesh^2)*dx. */
int pic_eval_field(pic_handle* h, const void* x, int mem_kind, const double* E_ext,
                   double* n, double* E_mesh, double* half_sum_E2_dx);

/* One environment step in three calls, each with its own external field: PIC.update_state_w_input_func
 * (pic.py:148-163), where the field is a function of the sub-stage state.  Stage k (1, 2, 3, in this order)
 * evaluates the force at q_k with E_ext (as in pic_step; NULL = none) and runs the sweep that kicks to p_k and
 * drifts to q_{k+1}; stage 3 also wraps x and refreshes n / E_mesh / phi / energies.  Between the calls
 * pic_get_particles returns the sub-stage state (q_{k+1} unwrapped, p_k) the caller's input function needs
 * (before stage 1: q_1 = x + (c_1 v) dt with c_1 = 0.5 / (2 - 2^(1/3)), formed by the caller).  pic_step and
 * pic_step_stage(1) are refused while a staged step is open; pic_reset / pic_set_particles abandon it. */
int pic_step_stage(pic_handle* h, int stage, const double* E_ext, int mem_kind);

/* Time integrator of every later step (additive to ABI 5: a handle starts with PIC_YOSHIDA4 and nothing else changes).  Each
 * scheme is PIC.update_state (pic.py:131-146) with symplectic_4th_order replaced by that function of src/env/integration.py,
 * in its operand order; E = gathered mesh field + E_ext, E_ext held over the step:
 *   PIC_SYMPLECTIC_EULER  1 force evaluation   p' = p + (1 (-E(q))) dt ; q' = q + (1 p') dt
 *   PIC_VERLET            2                    p+ = p + (0.5 (-E(q))) dt ; q' = q + (1 p+) dt ; p' = p+ + (0.5 (-E(q'))) dt
 *   PIC_FORWARD_EULER     1                    x' = x + dt v ; v' = v + dt (-E(x))
 * followed by the wrap and the post-step refresh, as Yoshida-4.  Every stepping entry runs every scheme, on both schedules and
 * with the recorder on or off; a step costs one pass over the particles (Verlet: one more per call).
 * pic_step_stage takes stages 1..S, S = evals_per_step: stage k evaluates the force with its E_ext and makes the sweep behind
 * it.  Between Verlet's stages 1 and 2 pic_get_particles returns (q' as drifted, not yet wrapped -- fixed32 positions are
 * wrapped by their format --, p+), the state its reference evaluates the second force at.
 * A change is refused (PIC_ESTATE) while a staged step is open, and drops the cached deposits as pic_invalidate does;
 * PIC_EINVAL for an unknown scheme. */
int pic_set_integrator(pic_handle* h, int scheme);
int pic_get_integrator(pic_handle* h, int* scheme, int* evals_per_step);

/* Whether the whole Yoshida-4 steps of the streaming schedule store sweep C's output.  With PIC_READONLY_ON sweep C
 * stores no particles and sweep D re-derives C's output from C's input and C's field tile, the same arithmetic on the same
 * operands: 80 bytes per float64 particle-step instead of 96, and the same bits.  PIC_READONLY_AUTO (the default) turns it on for
 * particle states of 256 MB and more, which stream from HBM.  pic_step_stage, the other integrators and the resident schedule
 * are not affected.  PIC_EINVAL for an unknown mode, or PIC_READONLY_ON where Ng leaves no LDS for the second field tile. */
enum { PIC_READONLY_AUTO = 0, PIC_READONLY_OFF = 1, PIC_READONLY_ON = 2 };
int pic_set_readonly_c(pic_handle* h, int mode);

/* Whether every second inner step of a call of whole Yoshida-4 steps stores its particles once.  With
 * PIC_ALTERNATE_ON such a step's sweeps B and D store nothing, its sweep C re-derives B and stores, and the next step's sweep B
 * re-derives D: three storing sweeps per pair of steps instead of four, 72 bytes per float64 particle-step instead of 80, and the
 * same bits.  In force only where the read-only sweep C is (pic_set_readonly_c), in a call of two or more steps without a feedback
 * law; a call's first and last step store as ever.  PIC_ALTERNATE_AUTO (the default) follows PIC_READONLY_AUTO.  PIC_EINVAL for an
 * unknown mode, or PIC_ALTERNATE_ON where Ng leaves no LDS for the second field tile. */
enum { PIC_ALTERNATE_AUTO = 0, PIC_ALTERNATE_OFF = 1, PIC_ALTERNATE_ON = 2 };
int pic_set_alternate_stores(pic_handle* h, int mode);

/* nsteps x PIC.update_state with the energies of every step kept, i.e. the E / PE traces PIC.simulate
 * returns (pic.py:175-223) without its particle snapshots: hist, host [nsteps][3][num_envs] float64 =
 * KE, PE, PE_reward after each step (total energy = KE + PE).  E_ext as in pic_step, constant over the steps.
 * No host synchronisation between the steps; returns when the history has arrived. */
int pic_step_history(pic_handle* h, const double* E_ext, int mem_kind, int nsteps, double* hist);

/* The same with the particle snapshots PIC.simulate returns as well (pic.py:175-223): snap, host
 * [nsteps][2][num_envs][N] of the particle dtype = positions (wrapped, in length units whatever the position format)
 * and velocities after each step; hist as in pic_step_history, or NULL.  The snapshots stay on the device until the
 * end of the call (PIC_ENOMEM if nsteps of them do not fit: record in several calls); in the resident schedule the
 * kernel writes them from its registers, one launch for all steps. */
int pic_step_snapshots(pic_handle* h, const double* E_ext, int mem_kind, int nsteps, void* snap, double* hist);

/* compute_E with everything it can return (src/env/util.py:73-116, return_all=True) and the shape-function
 * bookkeeping of compute_n / CIC / TSC (util.py:48-70, src/env/interpolate.py:4-44), on arbitrary positions.
 * x: [num_envs][N] particle dtype (host or device); E_ext: NULL or host [num_envs][Ng] float64.  Host outputs,
 * any may be NULL: E_part, phi_part [num_envs][N] (particle dtype) = E_mesh (incl. E_ext) and phi_mesh gathered
 * at the particles; n, E_mesh, phi_mesh [num_envs][Ng] float64 (phi in the mean-zero gauge); idx (int64) and
 * w (float64) [num_envs][3][N]: rows indx_l, indx_r, 0 / weight_l, weight_r, 0 for CIC and l, m, r for TSC.
 * Does not modify the environments' state. */
int pic_compute_E(pic_handle* h, const void* x, int mem_kind, const double* E_ext, void* E_part, void* phi_part,
                  double* n, double* E_mesh, double* phi_mesh, int64_t* idx, double* w);

/* Gaussian_Elimination_Periodic on the 3-point periodic Laplacian (src/env/solve.py:27-53 as called from
 * util.py:99) + E_mesh = -grad @ phi (util.py:100): rhs host [num_envs][Ng] float64, summing to zero per
 * environment as n - n0 does (otherwise the periodic problem has no solution) -> phi (mean zero), E_mesh; host,
 * either may be NULL. */
int pic_solve_poisson(pic_handle* h, const double* rhs, double* phi, double* E_mesh);

/* Device-side actuator, E_field (src/control/actuator.py:4-63).  pic_set_actuator uploads the host
 * mirror's basis tables, basis_cos / basis_sin [Ng][max_mode] float64 (they carry the reference's
 * linspace(0, L, Ng) mesh).  pic_step_actions runs nsteps x update_state under E_ext = basis_cos @ a[:M] +
 * basis_sin @ a[M:] (actuator.py:54-63), a = actions [num_envs][2*max_mode] float64 (host or device), held for the
 * nsteps.  The field is built inside the field phase of the kernels that use it: a controlled step costs no launch and
 * no mesh-sized copy more than an uncontrolled one. */
int pic_set_actuator(pic_handle* h, int max_mode, const double* basis_cos, const double* basis_sin);
int pic_step_actions(pic_handle* h, const double* actions, int mem_kind, int nsteps);

/* A rollout with a NEW action every step in one call -- the inner loop of the trainers (src/control/rl/ddpg.py:421-468,
 * ppo.py:307-372, sac.py:328-396) once the actions are known, and PIC.simulate with an action trajectory:
 * actions [nsteps][num_envs][2*max_mode] float64 (host or device); step s runs under actions[s].  Resident schedule: one launch
 * for all steps; streaming: three launches per step, as pic_step(nsteps).  hist: NULL, or host [nsteps][3][num_envs] = KE, PE,
 * PE_reward after each step (the call then returns when it has arrived; with NULL it is asynchronous like pic_step). */
int pic_step_actions_traj(pic_handle* h, const double* actions, int mem_kind, int nsteps, double* hist);

/* The same with the fields given on the mesh: PIC.simulate(E_external_traj) (pic.py:175-223, E_external_traj[i] of step i).
 * E_ext_traj [nsteps][num_envs][Ng] float64 (host or device); hist as above; snap: NULL, or the particle snapshots of
 * pic_step_snapshots. */
int pic_step_ext_traj(pic_handle* h, const double* E_ext_traj, int mem_kind, int nsteps, double* hist, void* snap);

/* nsteps of the linear feedback loop of run_feedback.py:130-168 on the device: before every step the actuator coefficients are
 * set to (-Re E_m, +Im E_m), m = 1..max_mode, of the Fourier modes (src/interpret/spectrum.py:16) of the mesh field the
 * previous step left (the current E_mesh for the first step) -- compute_E_k_spectrum, E_field.update_E, E_field.compute_E and
 * PIC.update_state of one loop iteration without leaving the device.  max_mode must be the actuator's (pic_set_actuator) and
 * at most 16.  actions_out: NULL, or host [nsteps][num_envs][2*max_mode] = the coefficients each step ran under (cos half, sin
 * half: the reference's coeff_cos / coeff_sin lists); hist as above.  Bit for bit what the host loop pic_get_modes ->
 * pic_step_actions gives. */
int pic_step_feedback(pic_handle* h, int max_mode, int nsteps, double* actions_out, double* hist);

/* nsteps of a linear feedback law with a gain of its own: before every step the modes
 * m = (Re E_1..Re E_M, Im E_1..Im E_M), M = max_mode, of the mesh field the previous step left (the current E_mesh for the first
 * step) are pic_step_feedback's, and the actuator coefficients are a = G m with the environment's own G:
 *     a[i] = sum over k = 0..2M-1 with G[i][k] != 0, in ascending k, of G[i][k] * m[k]
 * in float64, the first such product starting the sum and every further one added to it (no fused multiply-add); a row without
 * a non-zero entry gives +0.  With G = G0 = diag(-1 x M, +1 x M) every step is pic_step_feedback's, bit for bit.
 * gain: [num_envs][2M][2M] float64, row-major, in mem_kind memory (read in stream order).  max_mode: as pic_step_feedback.
 * actions_out, modes_out: NULL, or host [nsteps][num_envs][2M]: a and m of every step; hist as above.  Accepted wherever
 * pic_step_feedback is (every format, interpolation and integrator, recorder on or off) and, unlike it, while a tape is open:
 * the taped steps keep their m_t and the call's gain, so that pic_tape_backward[_feedback] differentiates through the law. */
int pic_step_feedback_gain(pic_handle* h, int max_mode, const double* gain, int mem_kind, int nsteps, double* actions_out,
                           double* modes_out, double* hist);

/* One iteration of a Gym-style loop in ONE call with ONE synchronisation (src/control/rl/ddpg.py:421-468, ppo.py, sac.py:
 * env.update_state(E) -> next_state = env.get_state() -> reward from the new state's electric energy): nsteps steps under
 * the given control -- E_ext [num_envs][Ng] on the mesh (util.py:102-103) or actions [num_envs][2*max_mode] actuator
 * coefficients (pic_step_actions), both host float64, at most one non-NULL -- then the particles (x, v: host [num_envs][N] in the
 * particle dtype, positions in length units) and the three energies (host [num_envs] each) of the state after them.  Any
 * output may be NULL.  Same results as pic_step / pic_step_actions followed by pic_get_particles and pic_get_energies,
 * which cost a synchronisation each (13-23 us of a 63 us iteration at the reference's N = 5000). */
int pic_step_observe(pic_handle* h, const double* E_ext, const double* actions, int nsteps, void* x, void* v,
                     double* KE, double* PE, double* PE_reward);

/* Rows 1..max_mode of compute_E_k_spectrum (src/interpret/spectrum.py:16) for the current E_mesh:
 * Ek[m] = fft(E_mesh)[m] / Ng * 2, re / im [num_envs][max_mode] float64 (host or device, any may be
 * NULL).  The feedback / behaviour-cloning action of run_feedback.py:133-135 and
 * src/control/rl/ddpg.py:369-371 is (-re, +im). */
int pic_get_modes(pic_handle* h, int max_mode, double* re, double* im, int mem_kind);

/* Phase-space histogram behind the KL diagnostic, estimate_f (src/control/objective.py:8-14):
 * counts[num_envs][nbins][nbins] (host, uint32) of the current particles on
 * np.histogram2d's bins for range [[0, L], [vmin, vmax]] -- same edge rules (edges lo + i*step,
 * last edge inclusive, out-of-range values dropped).  f = counts * n0 / dx / dv / N on the host. */
int pic_phase_histogram(pic_handle* h, int nbins, double vmin, double vmax, uint32_t* counts);

/* The KL cost built on it, Reward.compute_kl_divergence (src/control/rl/reward.py:43-46 -> estimate_KL_divergence,
 * objective.py:16-18), for every environment at once: kl[e] = sum_ij rel_entr(f_e[i][j], feq[i][j] + 1e-12) dx dv with
 * f_e = counts_e n0 / dx / dv / N, dx = L / nbins, dv = (vmax - vmin) / nbins; feq host [nbins][nbins] float64 (the target
 * density, estimate_f of the initial state), kl host [num_envs].  Histogram and reduction stay on the device. */
int pic_phase_kl(pic_handle* h, int nbins, double vmin, double vmax, const double* feq, double* kl);

/* Smoothed phase-space density and its KL cost, differentiable in the particles (additive to ABI 5).  For every
 * environment, with dx = L / nx and dv = (vmax - vmin) / nv:
 *     f[i][j] = n0 / (dx dv N) * sum_k Wx_i(x_k) Wv_j(v_k)        (estimate_f's normalisation, objective.py:12)
 * Wx is the periodic CIC weight on the bin centres (i + 1/2) dx of the stored, wrapped x; Wv the CIC weight on the centres
 * vmin + (j + 1/2) dv, the outer half-bins [vmin, vmin + dv/2) and (vmax - dv/2, vmax] giving their whole weight to the edge bin.
 * A particle outside [0, L] x [vmin, vmax] is dropped, as np.histogram2d drops it: sum f dx dv = n0 inside / N, the histogram's
 * mass.  A particle's four weights are integers that sum exactly to one particle unit 2^s (s from N: no bin can overflow), so f
 * is bitwise reproducible and does not depend on blocks_per_env, the schedule or the environment's place in the batch.
 *     kl = sum_ij rel_entr(f[i][j], feq[i][j] + 1e-12) dx dv        (estimate_KL_divergence, objective.py:16-18)
 * feq: the target, float64 in feq_mem_kind memory, [nx][nv] for every environment (feq_per_env = 0) or [num_envs][nx][nv] (1):
 * pic_phase_histogram's f, or this f of an initial state.  Float64 particles and positions only; 1 <= nx, nv <= 1024 and finite
 * vmin < vmax; anything else is PIC_EINVAL (the reason in pic_last_error).  Both entries return when their outputs have arrived. */
typedef struct pic_phase_spec {
  int32_t nx, nv;                  /* bins in x and in v, 1..1024 each                        */
  double  vmin, vmax;              /* velocity range; x spans [0, L]                          */
  const double* feq;               /* the KL's target, or NULL (the density alone)            */
  int32_t feq_per_env;             /* 0: feq [nx][nv]; 1: feq [num_envs][nx][nv]              */
  int32_t feq_mem_kind;            /* PIC_HOST | PIC_DEVICE                                   */
} pic_phase_spec;
/* kl [num_envs] (needs feq) and f [num_envs][nx][nv] of the current particles, in mem_kind memory; either may be NULL, not both. */
int pic_phase_kl_smooth(pic_handle* h, const pic_phase_spec* spec, int mem_kind, double* kl, double* f);
/* Vector-Jacobian product of kl: g_x, g_v [num_envs][N] float64 (dense, mem_kind memory; either may be NULL) receive
 * cot_kl[e] dkl_e/dx and cot_kl[e] dkl_e/dv of the current particles; cot_kl [num_envs] in mem_kind memory.  Needs feq.  The
 * derivative is the almost-everywhere one of the unquantised weights: dkl/df = (ln(f / (feq + 1e-12)) + 1) dx dv where f > 0
 * and 0 where f = 0, gathered at a particle's four bins with the CIC slopes -+1/dx in x and -+1/dv in v (0 in v in the clamped
 * half-bins; 0 for a dropped particle). */
int pic_phase_kl_smooth_vjp(pic_handle* h, const pic_phase_spec* spec, const double* cot_kl, int mem_kind, void* g_x, void* g_v);
/* Jacobian-vector product of kl, the forward mode of the same derivative (additive to ABI 5): for K directions
 * (1 <= K <= 8) d_kl[k][e] = sum_i dkl_e/dx_i d_x[k][e][i] + dkl_e/dv_i d_v[k][e][i] over the current particles, with exactly the
 * dkl/dx, dkl/dv that pic_phase_kl_smooth_vjp returns for cot_kl = 1.  d_x, d_v [K][num_envs][N] float64 (dense; either may be
 * NULL = 0), d_kl [K][num_envs], all in mem_kind memory.  Needs feq; spec is checked as pic_phase_kl_smooth_vjp checks it.
 * Every environment's particles are cut into chunks of 8192 (a constant); a chunk's products are summed in a fixed order and the
 * chunks' sums in ascending order, in float64: the result is bitwise reproducible, each direction is computed on its own, and
 * nothing depends on blocks_per_env, the schedule or the other environments of the batch.  Returns when d_kl has arrived. */
int pic_phase_kl_smooth_jvp(pic_handle* h, const pic_phase_spec* spec, int K, const void* d_x, const void* d_v, int mem_kind,
                            double* d_kl);

/* Per-kernel timing with HIP events on the handle's stream (bench.py's roofline leg).
 * kinds: 0..3 = sweeps A..D, 4 = field solve, 5 = auxiliary sweeps (refresh, first deposits), 6 = resident launches,
 * 7 = the particle sweeps of the other integrators (pic_set_integrator). ms_sum / launches are arrays of 8. */
int pic_profile(pic_handle* h, int enable);
int pic_profile_read(pic_handle* h, double* ms_sum, int64_t* launches);

/* Streaming ceiling of this device for the sweeps' access shape (read x and v, write x and v, same
 * grid, no arithmetic): bytes moved per second in GB/s, averaged over `repeats` launches on
 * scratch arrays of the handle's particle footprint.  bench.py reports it next to the 8 TB/s spec. */
int pic_stream_probe(pic_handle* h, int repeats, double* gbytes_per_s);

/* Run all further work of this handle on the caller's HIP stream (a hipStream_t, e.g. torch's current stream; NULL
 * is the device's default stream, which is what torch uses unless told otherwise) instead of the handle's own;
 * pic_own_stream switches back.  The previous stream is drained first.  With device-pointer inputs/outputs (pic_step,
 * pic_step_actions, pic_get_modes, pic_device_ptrs views) a control loop then stays stream-ordered with the caller's
 * kernels and needs no host synchronisation. */
int pic_set_stream(pic_handle* h, void* hip_stream);
int pic_own_stream(pic_handle* h);

/* 1 if pic_step runs the resident schedule on this handle, 0 for streaming sweeps (see blocks_per_env). */
int pic_schedule(pic_handle* h);

/* Particle states of 256 MB and more: x and v are two allocations, and pic_create times a streaming pass over (x, candidate
 * block for v) for a series of candidate blocks: on MI355X two arrays stream together at 6.05 TB/s when they lie in different
 * 32 GiB regions of HBM and at 5.25 TB/s when they share one.  The search stops sixteen readings after the best pair
 * seen is 10 % faster than the slowest seen (keeping the best of all), after 42 GiB and sixteen blocks walked without an improvement
 * (more than a 32 GiB region), or when a third of the device's free memory is held; no absolute rate enters.  It runs in LEGS of at most 100 ms
 * (or forty steps' worth of the handle being placed, if that is more: 160 ms at N = 4e6 x 64, 410 ms at N = 1e7 x 128 float32):
 * pic_create runs one; while the search has ended only for lack of time (outcome PIC_PLACED_TIMEOUT: on a device whose memory is
 * handed out for the first time hipMalloc clears it at 1.3-6 ms per 512 MB block, and the first block that pairs well with x can be
 * 31 GiB away), pic_reset / pic_reset_sampled -- which replace the particles anyway -- run another leg each, up to four in all, and
 * may move v.  What an earlier leg has cleared and released comes back in microseconds, so every leg gets further.  Once
 * pic_device_ptrs has handed out the addresses of x and v, v stays where it is and no further leg runs.  Candidate blocks are
 * allocated by a thread of the call's own (joined before the call returns) while the calling thread times them.
 * What a co-resident allocator (torch's caching allocator, another handle on another thread or rank of the same device) sees:
 * while pic_create runs, blocks of the state's size are allocated one after the other and up to a third of the free memory is
 * held; all but x and v are freed before it returns.  An allocation made by someone else in that window can fail for lack of
 * memory although it would fit a moment later: create large handles before filling the device, serialise creates per device, or
 * set pic_config.placement = PIC_PLACE_OFF (x | v in one block, no search, nothing held; config 2 then steps ~10 % slower when
 * the block falls into one region).  Results do not depend on the placement.
 * -> how many pairs were timed (1 with rates 0 = small state or search off, nothing timed), the read+write rate of the pair kept
 * and of the slowest pair seen, in GB/s, and the wall time the search took; any pointer may be NULL. */
int pic_placement_info(pic_handle* h, int* candidates, double* kept_gbytes_per_s, double* slowest_gbytes_per_s, double* seconds);

/* The same report with how the search ended and where its time went, all legs together (ABI 4).  malloc_seconds is the part that
 * memory handed out for the first time since the device came up makes expensive (the driver clears it inside hipMalloc: 1.3-6 ms per
 * 512 MB block against 20-150 us for memory that has been allocated and released before); timing_seconds the streaming passes
 * (filler, the leg's reference pair, one untimed + one timed pass per candidate); free_seconds the release of the blocks not kept. */
typedef struct {
  int32_t pairs_timed;             /* 0: no search */
  int32_t blocks;                  /* candidate blocks allocated in all (timed or walked over) */
  int32_t outcome;                 /* PIC_PLACED_* */
  int32_t legs;                    /* legs of the search run so far: pic_create runs one, resets may run more (see above) */
  double kept_gbytes_per_s;        /* read + write rate of the bare stream over (x, v kept) */
  double slowest_gbytes_per_s;     /* ... over the slowest pair timed */
  double seconds;                  /* wall time of the search, all legs */
  double malloc_seconds, timing_seconds, free_seconds;
} pic_placement;
int pic_placement_stats(pic_handle* h, pic_placement* out);

/* Rollout recorder (ABI 5): small reductions of the state, computed on the device after every `stride`-th step of ANY stepping
 * entry (pic_step, pic_step_history, pic_step_snapshots, pic_step_actions[_traj], pic_step_ext_traj, pic_step_feedback,
 * pic_step_observe, stage 3 of pic_step_stage) and held on the device until read -- the analyses the reference runs on a full
 * (2N, Nt) particle snapshot (src/interpret/landau.py, spectrum.py, the KL of run_ddpg.py:276-312) without the snapshot.
 * Steps are counted from pic_record_start over all calls; step k is recorded when k % stride == 0.  A recorded step ends like
 * the last step of a call and two kernels follow it (a particle pass for the histograms, one workgroup per environment for the
 * rest): particles, fields and energies are bit for bit those of the same calls without a recorder.  A record is bitwise
 * reproducible and does not depend on blocks_per_env or the schedule -- except KE, which is the step's own (pic_get_energies'):
 * its per-workgroup partial sums follow the sweep grid in the last bits.  Resets and pic_set_particles count no step and do not
 * end the recording.  A stepping call that would take the record count past `capacity` is refused (PIC_ENOMEM) before any
 * step runs.  Histogram edges are np.histogram / np.histogram2d's (as pic_phase_histogram). */
typedef struct pic_record_config {
  int32_t stride;                  /* >= 1 */
  int32_t n_modes;                 /* rows 0..n_modes-1 of fft(E_mesh) / Ng * 2 (spectrum.py:16); 0..Ng/2+1            */
  int32_t x_bins, v_bins;          /* marginal histograms of x on [0, L] and v on [vmin, vmax]; 0..4096, 0 = none        */
  int32_t phase_x_bins, phase_v_bins;  /* phase-space histogram behind entropy / KL, 1..4096 each, or both 0 = none     */
  double  vmin, vmax;              /* vmax > vmin */
  double  phase_dx, phase_dv;      /* f = counts * n0 / phase_dx / phase_dv / N; 0 = L / phase_x_bins, (vmax - vmin) / phase_v_bins */
  const double* feq;               /* NULL, or host [phase_x_bins][phase_v_bins]: the KL target (estimate_f normalisation) */
  int64_t capacity;                /* records held on the device, >= 1 */
} pic_record_config;

/* Host outputs of pic_record_read for records first..first+count-1; any pointer may be NULL.  Per record: step [count]
 * (int64, the step index k; 0 for a pic_record_now right after pic_record_start); per record and environment ([count][num_envs]):
 * KE, PE, PE_reward as pic_get_energies reports them, field_energy = sum(E_mesh^2) dx (landau.py:68), entropy =
 * -sum_{f>0} f ln f dx dv (landau.py:19-25, dx dv = phase_dx phase_dv), kl = sum rel_entr(f, feq + 1e-12) dx dv (pic_phase_kl;
 * NaN without feq or phase histogram), inside = particles with x in [0, L] and v in [vmin, vmax] (int64); re / im
 * [count][num_envs][n_modes]; x_hist [count][num_envs][x_bins], v_hist [count][num_envs][v_bins] (uint32). */
typedef struct pic_record_out {
  int64_t* step;
  double* KE;
  double* PE;
  double* PE_reward;
  double* field_energy;
  double* entropy;
  double* kl;
  double* re;
  double* im;
  uint32_t* x_hist;
  uint32_t* v_hist;
  int64_t* inside;
} pic_record_out;

int pic_record_start(pic_handle* h, const pic_record_config* cfg);   /* allocates (PIC_ENOMEM if capacity does not fit); PIC_ESTATE if on */
int pic_record_now(pic_handle* h);                                   /* append a record of the current state (e.g. t = 0) */
int pic_record_count(pic_handle* h, int64_t* n);                     /* records held (0 and PIC_OK when not recording) */
int pic_record_read(pic_handle* h, int64_t first, int64_t count, pic_record_out* out);   /* PIC_ESTATE when not recording */
int pic_record_stop(pic_handle* h);                                  /* frees; the records are gone */

/* Differentiable rollouts (the tape): the vector-Jacobian product of T Yoshida-4 steps from the state at pic_tape_start -- the
 * energies KE_t, PE_t, PE_reward_t of every step ([T][3][num_envs], pic_step_history's layout) and the final particles as
 * functions of every step's external field e_t (raw, or the actuator product of actions[t]) and of the initial particles.  The
 * derivative is the almost-everywhere one of the device's arithmetic: the wrap has slope 1, the CIC weights slopes -+1/dx.
 * Float64 particles and positions, PIC_ACC_FIX64, CIC and Yoshida-4 only (anything else: PIC_EINVAL, the reason in
 * pic_last_error).  While a tape is open pic_step, pic_step_history, pic_step_snapshots, pic_step_actions[_traj],
 * pic_step_ext_traj, pic_step_observe and pic_step_feedback_gain append to it (calls are cut behind every checkpoint step, as
 * the recorder cuts them: the same bits as untaped); a call that would take it past max_steps is refused with PIC_ENOMEM before
 * any step runs.  A gain-law call keeps its gain [num_envs][2M][2M] once and every step's modes m_t; the first one also
 * allocates the record of the law's steps (3 [max_steps][num_envs][2M] plus one [num_envs][Ng] of float64); both count in
 * `bytes` and against budget_bytes (PIC_ENOMEM beyond it);
 * pic_step_feedback, pic_step_stage, pic_reset, pic_reset_sampled, pic_set_particles, pic_set_actuator and pic_set_integrator
 * are refused with PIC_ESTATE.  DESIGN.md 7c; the stepwise reverse walk (pic_tape_walk_*): 7e. */
typedef struct pic_tape_config {
  int64_t max_steps;               /* >= 1: steps the tape can hold */
  int64_t checkpoint_every;        /* (x, v) kept every this many steps; 0 = the library chooses: ceil(sqrt(max_steps)), or
                                      the interval needing the fewest bytes when that exceeds budget_bytes */
  int64_t budget_bytes;            /* > 0: PIC_ENOMEM at pic_tape_start if the tape (checkpoints, fields, backward memory) needs more */
} pic_tape_config;

typedef struct pic_tape_info {
  int64_t steps;                   /* steps taped so far */
  int64_t checkpoint_every;
  int64_t bytes;                   /* device memory the tape holds */
  int64_t replay_mismatches;       /* particle values of the last backward's or tangent's replays that differ from the forward's (0 expected) */
  int64_t unit_retries;            /* repeated adjoint deposits (0: the unit of the adjoint deposits cannot overflow) */
  int64_t launches;                /* kernels the last backward or tangent enqueued */
  int64_t replay_bad_positions;    /* non-finite / out-of-range positions the last backward's or tangent's replay met (0 expected) */
} pic_tape_info;

int pic_tape_start(pic_handle* h, const pic_tape_config* cfg);   /* checkpoints the current state; PIC_ESTATE if a tape is open */
/* cot_hist [T][3][num_envs], cot_x / cot_v [num_envs][N] cotangents (each may be NULL = 0); outputs (each may be NULL):
 * g_ext [T][num_envs][Ng], g_actions [T][num_envs][2M] = B^T g_ext (needs pic_set_actuator), g_x0 / g_v0 [num_envs][N].  All in
 * mem_kind memory.  Asynchronous on the handle's stream for PIC_DEVICE; the handle's particles, fields, energies and cached
 * deposits are not touched.  The tape stays open (another backward with other cotangents may follow).  With PIC_HOST the call
 * waits and returns PIC_ESTATE if the replay differed from the taped forward (particles written through pic_device_ptrs while
 * taping); with PIC_DEVICE read replay_mismatches from pic_tape_stats. */
int pic_tape_backward(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, int mem_kind, double* g_ext,
                      double* g_actions, void* g_x0, void* g_v0);
/* pic_tape_backward of a tape that holds steps of pic_step_feedback_gain, with cotangents on their modes: cot_modes
 * [T][num_envs][2M] (NULL = 0; ignored on the other steps); modes_out [T][num_envs][2M]: the taped m_t (0 on the other steps).
 * The gradient includes the state path through the law (pic_tape_backward does too, with cot_modes = 0): a-bar_t = B^T e-bar_t,
 * m-bar_t = G^T a-bar_t + cot_modes_t, and J^T m-bar_t is a cotangent on the field step t started from.  g_actions holds
 * a-bar_t on every step; the gradient with respect to the gain of a call is sum over its steps of a-bar_t m_t^T (per environment),
 * which the caller forms from g_actions and modes_out. */
int pic_tape_backward_feedback(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, const double* cot_modes,
                               int mem_kind, double* g_ext, double* g_actions, void* g_x0, void* g_v0, double* modes_out);
int pic_tape_stats(pic_handle* h, pic_tape_info* out);           /* all zero when no tape is open; synchronises */
int pic_tape_stop(pic_handle* h);                                /* frees the tape */
/* The reverse pass one step at a time (a walk), so that a caller can put the vector-Jacobian product of its own
 * policy between two reverse steps.  pic_tape_walk_begin starts at step T (the tape's length); obs_modes M_o (1 <= M_o < Ng)
 * fixes the layout of the mode cotangents, [num_envs][2 M_o]: Re E_1..E_Mo then Im E_1..E_Mo (pic_get_modes' map).
 * pic_tape_walk_step reverses the next step t not yet walked (T-1, T-2, ...; its index in *step).  Its cotangents refer to what
 * step t produced (each may be NULL = 0): cot_energies [3][num_envs] (its row of pic_step_history's layout), cot_x / cot_v
 * [num_envs][N] on the state it left, cot_modes [num_envs][2 M_o] on the modes of the field it left (the observation of step
 * t+1).  Outputs (each may be NULL): g_ext [num_envs][Ng] = e-bar_t, g_actions [num_envs][2M] = B^T e-bar_t (needs an
 * actuator).  When t is the last step of its checkpoint segment the call first replays and compares the segment, as
 * pic_tape_backward does.  pic_tape_walk_end, once all T steps are walked, adds cot_x0 / cot_v0 on the tape's starting state and
 * cot_modes0 on the modes of the field there, and writes g_x0 / g_v0 [num_envs][N].  A tape with steps of pic_step_feedback_gain
 * is walked with the law's own term G^T a-bar_{t+1} added to cot_modes: zero injections give pic_tape_backward_feedback's bits.
 * PIC_DEVICE: asynchronous on the handle's stream.  PIC_HOST: a call with outputs waits, and pic_tape_walk_end returns
 * PIC_ESTATE if a replay differed from the taped forward.  Any step appended to the tape, pic_tape_start / stop / backward* and a
 * new pic_tape_walk_begin abandon a walk; walk_step and walk_end then return PIC_ESTATE, as they do without one. */
int pic_tape_walk_begin(pic_handle* h, int obs_modes, int mem_kind);
int pic_tape_walk_step(pic_handle* h, const double* cot_energies, const void* cot_x, const void* cot_v, const double* cot_modes,
                       int mem_kind, double* g_ext, double* g_actions, int64_t* step);
int pic_tape_walk_end(pic_handle* h, const void* cot_x0, const void* cot_v0, const double* cot_modes0, int mem_kind, void* g_x0,
                      void* g_v0);
/* Forward mode of the tape: the Jacobian-vector product of the T steps taped so far in K directions at once
 * (1 <= K <= 8), with the almost-everywhere derivative of the backward.  Inputs (each may be NULL = 0): d_ext [K][T][num_envs][Ng]
 * tangents of every step's external field e_t, or d_actions [K][T][num_envs][2M] tangents of the actions, mapped through the
 * actuator basis as e_t is (needs an actuator set before pic_tape_start; at most one of the two); d_x0 / d_v0 [K][num_envs][N]
 * on the tape's starting state.  Outputs (each may be NULL): d_hist [K][T][3][num_envs] the tangents of KE, PE, PE_reward
 * (pic_step_history's layout per direction), d_x / d_v [K][num_envs][N] of the final particles, d_E_mesh [K][T][num_envs][Ng] of
 * every step's post-step E_mesh.  Each direction is computed on its own (K directions in one call equal K calls bit for bit);
 * results do not depend on blocks_per_env, the checkpoint interval, the schedule or the other environments of the batch.  All in
 * mem_kind memory, as pic_tape_backward: PIC_DEVICE is asynchronous on the handle's stream; PIC_HOST waits and returns
 * PIC_ESTATE if a replay differed from the taped forward.  The tape stays open; the handle's particles, fields, energies and
 * cached deposits are not touched, and a later pic_tape_backward gives the same bits as without this call.  It abandons a walk
 * in progress; pic_tape_stats then reports this call's replay counts.  The first call with K directions allocates their
 * working memory ((2 K num_envs ld + 2 K num_envs Ng + 4 K num_envs) * 8 bytes, each part rounded up to 256), which counts in
 * `bytes` and against budget_bytes (PIC_ENOMEM, the tape still usable) and is freed by pic_tape_stop.  No tape open, or a tape
 * holding steps of pic_step_feedback_gain (forward mode through the gain law is not built): PIC_ESTATE.  K outside 1..8, both
 * d_ext and d_actions, or a bad mem_kind: PIC_EINVAL.  T = 0: d_x / d_v are d_x0 / d_v0 and nothing else is written. */
int pic_tape_tangent(pic_handle* h, int K, const double* d_ext, const double* d_actions, const void* d_x0, const void* d_v0,
                     int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh);
/* The smoothed phase-space KL of pic_phase_kl_smooth after EVERY taped step, forward and adjoint (additive to
 * ABI 5): with it the running cost sum_t KL~_t of the reference's trainers is differentiable next to the energy traces.
 * pic_tape_kl_start attaches it to an open tape that holds no step and no KL yet (else PIC_ESTATE).  spec is checked as
 * pic_phase_kl_smooth checks it and needs feq (else PIC_EINVAL); the tape takes its own device copy of feq, so the caller's may
 * go away.  It allocates, with nb = nx nv, E = num_envs and every part rounded up to 256 bytes,
 *     8 ((feq_per_env ? E : 1) nb  +  E nb  +  E nb  +  max_steps E  +  max_steps E)   bytes
 * (the target, the integer sums, the cotangent grid, the KL trace and its cotangents), which count in pic_tape_info.bytes and
 * against budget_bytes and are freed by pic_tape_stop.  If they do not fit, or take the tape past budget_bytes: PIC_ENOMEM, and
 * the tape stays usable without a KL.
 * From then on every stepping call is cut behind every step (as the recorder cuts with stride 1: particles, fields and energies
 * are bit for bit those of the same calls without a KL, or without a tape) and two kernels write kl[t][e], bit for bit what
 * pic_phase_kl_smooth returns when called after step t.  pic_tape_kl copies the trace of the T steps taped so far,
 * kl [T][num_envs] in mem_kind memory (PIC_HOST waits; PIC_DEVICE is asynchronous on the handle's stream).
 * pic_tape_kl_cot stores cotangents on it: cot_kl [nsteps][num_envs] in mem_kind memory for steps first_step ..
 * first_step + nsteps - 1, or NULL to clear those rows.  Rows persist until they are overwritten or cleared, and
 * pic_tape_kl_start leaves all clear.  Every later pic_tape_backward, pic_tape_backward_feedback and pic_tape_walk_step adds
 * cot_kl[t] dKL~_t/d(x, v) to the adjoint state when it reverses a step t that holds a row (three more kernels per such step,
 * counted in `launches`; the derivative is pic_phase_kl_smooth_vjp's); a step without a row costs nothing, so a tape with a KL
 * and no rows set gives the gradients of a plain tape bit for bit.  The call does not abandon a walk, but rows of steps a walk
 * in progress has already reversed are refused with PIC_ESTATE; rows outside [0, T) or a bad mem_kind are PIC_EINVAL; no tape
 * with a KL open is PIC_ESTATE (pic_tape_kl too).  Gradients with KL cotangents are bitwise reproducible and do not depend on
 * blocks_per_env, the checkpoint interval, the schedule or the other environments of the batch.
 * Forward mode: pic_tape_tangent works on such a tape and ignores the KL; pic_tape_tangent_kl returns the KL's tangents too. */
int pic_tape_kl_start(pic_handle* h, const pic_phase_spec* spec);
int pic_tape_kl(pic_handle* h, int mem_kind, double* kl);
int pic_tape_kl_cot(pic_handle* h, const double* cot_kl, int mem_kind, int64_t first_step, int64_t nsteps);
/* pic_tape_tangent with the tangents of the per-step KL (additive to ABI 5): the arguments of pic_tape_tangent and
 * d_kl [K][T][num_envs] in mem_kind memory, d_kl[k][t][e] = the derivative of kl[t][e] (pic_tape_kl) along direction k, the
 * almost-everywhere derivative pic_tape_kl_cot's reverse pass uses: forward and reverse are dual.  d_kl = NULL is pic_tape_tangent
 * itself (same kernels, same bits; a KL on the tape is ignored).  With d_kl the tape must hold a KL (pic_tape_kl_start), else
 * PIC_ESTATE; every other refusal is pic_tape_tangent's, a tape with steps of pic_step_feedback_gain included.  Every step then
 * costs 4 more kernels, counted in `launches`: behind the third sub-stage of step t the deposit and the finishing kernel on the
 * replayed state the step left (unit cotangents), pic_phase_kl_smooth_jvp's pass over the particles against the tangent state,
 * and the sum of its chunks.  All other outputs are bit for bit pic_tape_tangent's, and d_kl shares their guarantees: K
 * directions in one call equal K calls, and nothing depends on blocks_per_env, the checkpoint interval, the schedule or the other
 * environments of the batch (the sums' order: pic_phase_kl_smooth_jvp).  The KL trace, the rows of pic_tape_kl_cot and a later
 * pic_tape_backward* are untouched.  The first call with d_kl allocates, with E = num_envs and each part rounded up to 256 bytes,
 *     8 (E  +  8 E ceil(ceil(N / 2) / 4096))   bytes
 * (the unit cotangents and the chunks' sums of 8 directions), which count in `bytes` and against budget_bytes (PIC_ENOMEM, the
 * tape still usable) and are freed by pic_tape_stop.  T = 0: nothing is written to d_kl. */
int pic_tape_tangent_kl(pic_handle* h, int K, const double* d_ext, const double* d_actions, const void* d_x0, const void* d_v0,
                        int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh, double* d_kl);

/* ---- Fluid moments on the mesh (additive to ABI 5) --------------------------------------------------------------
 * The density, momentum density and twice the kinetic-energy density of the stored (wrapped) particles on the handle's N_mesh
 * nodes, with s = n0 L / (N dx) and W the handle's own shape function (CIC or TSC; the cell is the forward's; the weights are
 * the forward's for float64 particles, and for float32 / fixed32 particles the shape function evaluated in double at the held
 * position's offset in that cell, because the forward's float32 weights carry up to ulp(L) / dx of cancellation error):
 *     m0_j = s sum_i W_j(x_i)        m1_j = s sum_i W_j(x_i) v_i        m2_j = s sum_i W_j(x_i) v_i^2
 * (mean velocity u = m1 / m0, temperature T = m2 / m0 - u^2).  pic_moments fills m [num_envs][3][N_mesh] float64 in mem_kind
 * memory for every particle format (PIC_HOST waits; PIC_DEVICE is asynchronous on the handle's stream); PIC_ESTATE before
 * pic_reset and during a staged step.  All three are 64-bit integer sums: m0 in the forward's fixed-point units, so that on a
 * float64 handle with the fixed-point accumulator it equals pic_get_fields' n of a fresh state bit for bit; m1 and m2 in units
 * taken from the environment's max |v| < 2^e, 2^(e + b - 61) and 2^(2e + b - 61) with 2^b >= N.  Every term is rounded to nearest
 * in its unit, so m1 and m2 of a node are off by up to half a unit per particle that touches it, whatever that node's own
 * velocities: one fast particle coarsens m1 and m2 of its whole environment (and of no other), which resolve N 2^-61 of
 * N max |v| and N max |v|^2, not of the node's own value.  Scaling every velocity of an environment by 2^k scales m1 by 2^k and m2
 * by 2^(2k) bit for bit while every result stays a normal double.  The result does not depend on blocks_per_env, the schedule,
 * accum_dtype or the environment's place in the batch.  An environment at rest has
 * m1 = m2 = +0; one with a non-finite velocity has NaN in m1 and m2 (m0 and the other environments are unaffected); with
 * max |v| >= 2^511, m2 is +inf.  Particles, fields, energies and pic_bad_count are untouched.  N_mesh above 2728 is PIC_EINVAL
 * (three meshes of 64-bit sums in 64 KB of LDS).  The first call allocates 8 (6 num_envs N_mesh + num_envs) bytes.
 * pic_moments_vjp: with cot_m [num_envs][3][N_mesh], g_x and g_v [num_envs][N] float64 (either may be NULL) receive the gradient
 * of sum cot_m . m with respect to the current particles, the almost-everywhere derivative of the CIC weights (as the tape's,
 * with the unquantised weights): with j, jr the nodes and w_l, w_r the weights of particle i,
 *     g_x_i = s (slope(c0) + v_i slope(c1) + v_i^2 slope(c2)),       slope(c) = (c[jr] - c[j]) / dx
 *     g_v_i = s ((w_l c1[j] + w_r c1[jr]) + 2 v_i (w_l c2[j] + w_r c2[jr])).
 * PIC_EINVAL for float32 / fixed32 particles and for TSC.
 * pic_tape_moments_cot stores cotangents on the moments of the states of an open tape: cot_m [nsteps][num_envs][3][N_mesh] in
 * mem_kind memory for rows first_step .. first_step + nsteps - 1, or NULL to clear those rows; row s belongs to the state step s
 * left, row -1 to the state at the start of the tape.  Rows persist until they are overwritten or cleared.  Every later
 * pic_tape_backward, pic_tape_backward_feedback and pic_tape_walk_step adds the gradient above, at the replayed state, to the
 * adjoint state when it reverses a step whose row is set (one more kernel, counted in `launches`), and pic_tape_walk_end (or the
 * end of a backward) adds row -1 at the first checkpoint; a tape with no row set launches nothing new and its gradients keep
 * their bits.  The first call that sets a row allocates 8 (max_steps + 1) num_envs 3 N_mesh bytes (rounded up to 256), which
 * count in pic_tape_info.bytes and against budget_bytes (PIC_ENOMEM, the tape still usable) and are freed by pic_tape_stop.
 * No open tape: PIC_ESTATE; rows outside [-1, T) or a bad mem_kind: PIC_EINVAL; rows of steps a walk in progress has already
 * reversed: PIC_ESTATE (the call does not abandon the walk). */
int pic_moments(pic_handle* h, int mem_kind, double* m);
int pic_moments_vjp(pic_handle* h, const double* cot_m, int mem_kind, void* g_x, void* g_v);
int pic_tape_moments_cot(pic_handle* h, const double* cot_m, int mem_kind, int64_t first_step, int64_t nsteps);

/* ---- Forward mode of the fluid moments (additive to ABI 5) -------------------------------------------------------
 * pic_moments_jvp: the directional derivative of pic_moments along K (1..8) tangents of the current particles, d_x and d_v
 * [K][num_envs][N] float64 in mem_kind memory (either may be NULL: 0), into d_m [K][num_envs][3][N_mesh].  float64 particles and
 * CIC only (PIC_EINVAL otherwise, and for N_mesh above 2728); PIC_ESTATE before pic_reset and during a staged step.  The
 * derivative is pic_moments_vjp's, transposed term by term: with iota = d_x_i / dx, particle i adds to its nodes j and jr
 *     dm0:  -iota                          +iota
 *     dm1:  w_l d_v_i - iota v_i           w_r d_v_i + iota v_i
 *     dm2:  2 w_l v_i d_v_i - iota v_i^2   2 w_r v_i d_v_i + iota v_i^2
 * times s, so that sum c . pic_moments_jvp(u) = pic_moments_vjp(c) . u, sum_j dm0_j = 0 (exactly in the integer sums: both halves
 * are one rounded integer; each float64 dm0_j then carries the rounding of its conversion and of the product by s, so
 * |sum_j dm0_j| <= 2^-52 sum_j |dm0_j|) and sum_j dm2_j N dx / (2 n0 L) = sum_i v_i d_v_i.  Every term is a 64-bit integer in the
 * unit 2^(e + b - 61), 2^b >= N,
 * where 2^e exceeds the largest bound |iota|, |d_v| + |iota v|, 2 |v d_v| + |iota| v^2 on one term of that moment, direction and
 * environment: the result is bitwise reproducible, K directions in one call equal K calls, and nothing depends on blocks_per_env,
 * the schedule or the environment's place in the batch.  A moment whose terms are all zero is +0; a non-finite tangent or velocity
 * gives NaN in the moments it reaches, of that direction and environment only.  The call allocates its working memory
 * (8 (3 K num_envs N_mesh + 3 K num_envs) bytes, plus device copies of host arrays) and waits for the stream before it lets go
 * of it; the kernels run on the handle's stream.  Particles, fields, energies, pic_moments' own accumulators and the tape are
 * untouched.
 * pic_tape_moments_start turns on a trace of the moments on an open tape that holds no step yet (PIC_ESTATE otherwise, and for a
 * second start): behind every taped step the three kernels of pic_moments write row t of [max_steps][num_envs][3][N_mesh], so row
 * t is bit for bit what pic_moments returns after step t.  Like a tape with a KL, such a tape runs its steps one launch at a time;
 * the steps keep their bits.  The trace takes 8 max_steps num_envs 3 N_mesh bytes (rounded up to 256), which count in
 * pic_tape_info.bytes and against budget_bytes (PIC_ENOMEM, the tape still usable without a trace) and are freed by
 * pic_tape_stop.  pic_tape_moments copies the rows of the steps taped so far to m in mem_kind memory (PIC_HOST waits).
 * pic_tape_tangent_moments is pic_tape_tangent_kl with d_moments [K][T][num_envs][3][N_mesh]: d_moments[k][t] = pic_moments_jvp
 * of the state step t left along direction k's tangent of that state.  d_moments = NULL is pic_tape_tangent_kl itself.  It needs
 * no trace on the tape.  Every step costs 3 more kernels, counted in `launches` (11 + 3 per step; + 4 with d_kl), behind the third
 * sub-stage next to the KL's.  All other outputs keep their bits, and d_moments shares their guarantees (K, checkpoint interval,
 * schedule, batch).  The first call with d_moments allocates, each part rounded up to 256 bytes,
 *     8 (24 num_envs N_mesh  +  24 num_envs)   bytes
 * (the integer sums and max words of 8 directions), which count in `bytes` and against budget_bytes and are freed by
 * pic_tape_stop.  Tapes with steps of pic_step_feedback_gain stay refused. */
int pic_moments_jvp(pic_handle* h, int K, const void* d_x, const void* d_v, int mem_kind, double* d_m);
int pic_tape_moments_start(pic_handle* h);
int pic_tape_moments(pic_handle* h, int mem_kind, double* m);
int pic_tape_tangent_moments(pic_handle* h, int K, const double* d_ext, const double* d_actions, const void* d_x0, const void* d_v0,
                             int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh, double* d_kl, double* d_moments);

/* Forward mode through closed loops (additive to ABI 5): the T steps on the tape one at a time, forward in time, in
 * K <= 8 directions, so that the action tangent of a step can come from the field tangent the step before left -- through the
 * gain law on the device, or through any policy's Jacobian-vector product on the caller's side between two steps.  Dual to
 * pic_tape_walk_* and pic_tape_backward_feedback; pic_tape_tangent* keep refusing tapes with steps of pic_step_feedback_gain.
 * pic_tape_tangent_walk_begin: 1 <= K <= 8; obs_modes M_o = 0 (no observation) or 1 <= M_o < N_mesh; d_x0 / d_v0
 * [K][num_envs][N] tangents of the tape's starting particles (NULL = 0); d_gain [K][num_envs][2M][2M] (NULL = 0) the tangent of
 * the gain of every gain-law step on the tape (PIC_EINVAL on a tape without one; tapes whose gains need different tangents inject
 * dG m_t through d_actions instead).  It computes the tangent of the field the tape started from, dE_0 = K drho(x_0; dx_0), by
 * a tangent deposit at the stored x_0, and from it d_modes0 [K][num_envs][2 M_o] (per environment Re E_1..E_Mo, then Im: the map
 * of pic_get_modes and of pic_tape_walk_*'s mode cotangents) and the law's dm_0.
 * pic_tape_tangent_walk_step advances the next step s (0, 1, ...; its index in *step).  d_ext [K][num_envs][N_mesh] or d_actions
 * [K][num_envs][2M] (at most one) is this step's injection.  On a gain-law step the device forms
 * da_s = (G_s dm_s + dG m_s) + d_actions with the taped m_s and G_s (G dm by the forward law's rule: the non-zero G[i][k] in
 * ascending k; dG m as a plain ascending sum); d_ext there is PIC_EINVAL.  Outputs, each optional, of the state step s left:
 * d_energies [K][3][num_envs], d_modes [K][num_envs][2 M_o] (the observation o_{s+1}), d_actions_out [K][num_envs][2M] (the
 * total applied), d_x / d_v [K][num_envs][N], d_E_mesh [K][num_envs][N_mesh].  The first step of a checkpoint segment replays
 * and compares the segment, as pic_tape_tangent does.  pic_tape_tangent_walk_end, valid once all T steps are walked, returns the
 * final d_x / d_v; in PIC_HOST memory it returns PIC_ESTATE if a replay differed from the taped forward.
 * pic_tape_tangent_feedback is the whole tape in one call through the same per-step function: d_actions [K][T][num_envs][2M]
 * injections, d_modes [K][T][num_envs][2M] the tangents of the law's own modes m_t (zero on other steps), d_actions_out
 * [K][T][num_envs][2M], the others in pic_tape_tangent's layouts.  On a tape without law steps and with equal inputs, d_hist,
 * d_E_mesh, d_x and d_v are pic_tape_tangent's bit for bit; with zero injections the walk and the one-call entry give the same
 * bits.  All outputs are bitwise reproducible and independent of K's grouping, checkpoint_every, blocks_per_env, the schedule
 * of the forward and the batch.  Every step costs pic_tape_tangent's 11 kernels plus one small one (the modes; none without a law
 * step or an observation) and one more where a caller's d_actions arrives; all counted in `launches`.
 * Any step appended to the tape, pic_tape_start / stop / backward*, pic_tape_tangent*, pic_tape_walk_begin and a new begin abandon
 * a tangent walk; a tangent walk abandons a reverse walk (both replay into the segment buffer).  walk_step / walk_end without a
 * live walk, or walk_step past T, return PIC_ESTATE.  The working rows, each part rounded up to 256 bytes,
 *     8 K (num_envs N_mesh + 3 num_envs + 2 M_o num_envs + 2 (2M num_envs) + 4 M^2 num_envs + num_envs max(N_mesh, 2M))   bytes
 * next to pic_tape_tangent's block, count in `bytes` and against budget_bytes.  The tangents of the per-step KL and of the
 * moments are not available step by step. */
int pic_tape_tangent_walk_begin(pic_handle* h, int K, int obs_modes, const void* d_x0, const void* d_v0, const double* d_gain,
                                int mem_kind, double* d_modes0);
int pic_tape_tangent_walk_step(pic_handle* h, const double* d_ext, const double* d_actions, int mem_kind, double* d_energies,
                               double* d_modes, double* d_actions_out, void* d_x, void* d_v, double* d_E_mesh, int64_t* step);
int pic_tape_tangent_walk_end(pic_handle* h, int mem_kind, void* d_x, void* d_v);
int pic_tape_tangent_feedback(pic_handle* h, int K, const double* d_gain, const void* d_x0, const void* d_v0,
                              const double* d_actions, int mem_kind, double* d_hist, double* d_modes, double* d_actions_out,
                              void* d_x, void* d_v, double* d_E_mesh);

/* Copies of whole environments on the device: afterwards environment e of dst is environment map[e] of src --
 * particles (the whole padded row, byte for byte), n, E_mesh, phi, the energies and the cached first deposit of the next step
 * (the resident schedule's hand-over mesh and carried cells included), so that a copy continues bit for bit like its source.
 * map: dst->num_envs entries in mem_kind memory.
 *   src == dst (fork): map[e] == e keeps environment e; every other entry must name a kept environment (map[map[e]] == map[e]),
 *     so no source is overwritten while it is read.  map = NULL is refused.
 *   src != dst (broadcast / restore): every environment of dst is overwritten; 0 <= map[e] < src->num_envs; map = NULL is the
 *     identity and needs equal num_envs.  The handles must agree in N, Ng, L, n0, dt, particle and position dtype, interpol,
 *     accumulator, integrator and device (PIC_EINVAL names the field); num_envs, blocks_per_env and the schedule may differ.
 *     Where they lay a cache out differently, dst's cache is dropped as pic_invalidate drops it (the same bits afterwards).
 * PIC_ESTATE if src has no state, if either handle is inside a staged step, if dst has a tape open, or if a device map meets
 * a dst without state (an entry the kernels refuse keeps its environment, so there must be one to keep).  A recorder on dst stays
 * on and counts no step; pic_bad_count of either handle is unchanged; dst has state afterwards.
 * Asynchronous on dst's stream; between two handles dst's stream first waits for the work queued on src's, and src's stream then
 * waits for the copy.  A host map is checked on the host (PIC_EINVAL, nothing copied).  A device map is checked by the kernels
 * without a host synchronisation: an entry out of range or against the keep rule leaves its environment as it was and adds 1 to
 * a counter of dst, which pic_copy_envs_rejected reads (it waits for the stream; cumulative since pic_create). */
int pic_copy_envs(pic_handle* dst, pic_handle* src, const int32_t* map, int mem_kind);
int pic_copy_envs_rejected(pic_handle* dst, int64_t* count);

/* ---- Closed loops under an MLP policy on the device (additive to ABI 5) -----------------------------------------
 * a = pi(o): the observation o = (Re E_1..Re E_Mo, Im E_1..Im E_Mo) is what pic_get_modes(Mo) returns for the same field, bit for
 * bit (the layout of the gain law's m); pi is an MLP of 1..4 linear layers, evaluated by one workgroup per environment.
 *   h_0 = o, or o * obs_scale element by element.
 *   layer l: y_i = b_i; then, for k ascending, y_i = y_i + W[i][k] * h_l[k] -- the product rounded, then the sum, no fused
 *     multiply-add.  Behind every layer but the last h_{l+1} = tanh(y) (the device's float64 tanh, PIC_ACT_TANH) or
 *     y > 0 ? y : +0.0 (PIC_ACT_RELU).
 *   z = the last layer's y.  With noise: u = z + std_i * eps_i (the product rounded first; std NULL = 1); without: u = z.
 *   squash 0: a = u.  squash 1: a = action_scale * tanh(u).
 * The library draws nothing: eps is the caller's, so a rollout is reproducible bit for bit. */
#define PIC_ACT_TANH 0
#define PIC_ACT_RELU 1
typedef struct pic_policy {
  int obs_modes;           /* Mo, 1 <= Mo <= 64 and Mo < Ng */
  int n_layers;            /* 1..4 linear layers */
  int width[5];            /* width[0] = 2 Mo, width[n_layers] = 2 max_mode of pic_set_actuator, every width 1..256 */
  int activation;          /* PIC_ACT_TANH or PIC_ACT_RELU behind every layer but the last */
  int squash;              /* 0: a = u;  1: a = action_scale * tanh(u) */
  int per_env;             /* 0: one parameter vector for all environments;  1: params is [num_envs][P] */
  double action_scale;
  const double* params;    /* per layer l: W_l [width[l+1]][width[l]] row-major, then b_l [width[l+1]];  P doubles in all */
  const double* obs_scale; /* NULL, or [2 Mo] */
} pic_policy;

/* pic_policy_eval: the policy once, for every environment, on obs [num_envs][2 Mo] or (obs NULL) on the modes of the current
 * E_mesh; the state is not touched (allowed while a tape is open).  noise: [num_envs][2M] or NULL; std: [2M] or NULL.
 * obs_out [num_envs][2 Mo] (the observation before obs_scale), pre_out (u) and actions_out (a) [num_envs][2M]: any may be NULL.
 *
 * pic_step_policy: nsteps closed-loop steps without returning to the host between them.  Step s is pic_policy_eval on the field
 * the previous step left (the current E_mesh for the first step), then one step exactly as pic_step_actions(a_s on the device, 1)
 * makes it: the call gives the bits of that host loop, and is accepted wherever pic_step_actions is (every particle format, CIC
 * or TSC, every integrator, both schedules, recorder on or off).  One policy launch plus one step's launches per step; the
 * actions of all steps lie in one device buffer of the handle, a row per step.  noise: [nsteps][num_envs][2M] or NULL;
 * obs_out [nsteps][num_envs][2 Mo], pre_out, actions_out [nsteps][num_envs][2M]; hist: NULL, or host [nsteps][3][num_envs] as
 * pic_step_actions_traj.
 *
 * mem_kind covers params, obs_scale, obs, noise, std and the three per-step outputs (all float64); inputs are read in stream
 * order.  With PIC_HOST outputs (or hist) the call waits once, at the end; with PIC_DEVICE and no hist it is asynchronous on the
 * handle's stream.
 * PIC_ESTATE: no actuator (pic_set_actuator); before pic_reset (pic_policy_eval: only with obs NULL); pic_step_policy while a tape
 * is open (the gradient through the policy would be missing: pic_tape_step_policy below is the taped entry; a torch policy on the
 * tape is the route for other networks) or inside a staged step.  PIC_EINVAL, with the reason in pic_last_error, before anything is enqueued and with the state untouched: a NULL
 * policy or params, n_layers outside 1..4, Mo outside 1..64 or >= Ng, a width outside 1..256, width[0] != 2 Mo,
 * width[n_layers] != 2M, an unknown activation, squash or per_env other than 0 / 1, a bad mem_kind, nsteps < 0. */
int pic_policy_eval(pic_handle* h, const pic_policy* p, const double* obs, const double* noise, const double* std, int mem_kind,
                    double* obs_out, double* pre_out, double* actions_out);
int pic_step_policy(pic_handle* h, const pic_policy* p, const double* noise, const double* std, int mem_kind, int nsteps,
                    double* obs_out, double* pre_out, double* actions_out, double* hist);

/* ---- Policy gradients on the device (additive to ABI 5) -----------------------------------------------------------
 * The vector-Jacobian product of the evaluation above, for one environment and one evaluation: from the recorded observation o,
 * the recorded u (pre) and a cotangent a-bar on the action.
 *   1. h_0 .. h_{L-1} are recomputed from o exactly as the forward computes them (the same bits).
 *   2. squash 0: u-bar_i = a-bar_i.  squash 1: t = tanh(u_i), s = action_scale * (1.0 - t*t), u-bar_i = a-bar_i * s.  Noise and
 *      std are additive, so z-bar = u-bar; g_pre = u-bar, and the caller forms d/d std as sum g_pre * eps.
 *   3. delta = z-bar.  For l = L-1 .. 0:  g_b_l[i] = delta[i];  g_W_l[i][k] = delta[i] * h_l[k];
 *      h-bar_l[k] = sum_i W_l[i][k] * delta[i], i ascending, the product rounded before the sum (no fused multiply-add), the
 *      first product starting the sum;  if l > 0: delta[k] = h-bar_l[k] * d[k], with d = 1.0 - h*h (tanh; h the activation) or
 *      h > 0 ? 1.0 : 0.0 (relu; h > 0 exactly where the pre-activation is).
 *   4. o-bar[k] = h-bar_0[k], times obs_scale[k] if given.
 * Parameter gradients are summed per environment over the policy steps in the order a reverse pass meets them (t descending),
 * each sum as g = g + term with the first term starting it; with per_env the result is [num_envs][P], with shared parameters the
 * per-environment sums are then added in ascending environment order.  No floating-point atomics: the result does not depend on
 * blocks_per_env, the checkpoint interval, the schedule or the launch geometry.
 *
 * pic_policy_vjp: the VJP once for every environment, on obs [num_envs][2 Mo], pre [num_envs][2M] (NULL allowed only with
 * squash == 0) and cot_actions [num_envs][2M]; g_params [P] or [num_envs][P] (per_env), g_obs [num_envs][2 Mo], g_pre
 * [num_envs][2M], each may be NULL.  The state is not touched (allowed while a tape is open, needs no pic_reset).  Checked like
 * pic_policy_eval: PIC_EINVAL with the reason, nothing enqueued.  With PIC_HOST the call waits; with PIC_DEVICE it is asynchronous.
 *
 * pic_tape_step_policy: pic_step_policy appended to an open tape (PIC_ESTATE without one).  Particles, fields, energies and the
 * three outputs have the bits of the untaped call.  The tape keeps one copy of the call's parameters and obs_scale, every step's
 * o_t, u_t and a_t, and which call each step belongs to; e_t = B a_t goes on the tape as an actions step's, so the replay compares
 * bit for bit.  max_steps and budget_bytes are checked before any step runs (PIC_ENOMEM; the record counts in
 * pic_tape_info.bytes).  All policy calls of one tape must agree in widths, activation, squash, per_env and Mo (PIC_EINVAL);
 * they may be mixed with pic_step_actions* and pic_step_feedback_gain calls.  pic_step_policy itself stays refused under a tape.
 *
 * pic_tape_backward_policy: pic_tape_backward on a tape with policy steps.  cot_actions [T][num_envs][2M] and cot_obs
 * [T][num_envs][2 Mo] (each may be NULL) are direct cotangents on the policy steps' actions and observations (rows of other steps
 * are ignored).  At a policy step t, once e-bar_t is complete: a-bar_t = B^T e-bar_t + cot_actions_t; the VJP above; m-bar_t = o-bar_t + cot_obs_t; E-bar_t = J^T m-bar_t joins the refresh adjoint of
 * step t-1, or reaches x_0 through the tape's starting field for t = 0.  g_params: the sum over all policy steps of the tape;
 * g_pre, g_actions [T][num_envs][2M] and g_obs [T][num_envs][2 Mo] hold u-bar_t, a-bar_t and o-bar_t, zero on the other steps.
 * Every output may be NULL.  PIC_ESTATE on a tape without policy steps.
 * B^T e-bar_t is summed twice, as pic_tape_backward_feedback sums it for a step of the gain law: in ascending mesh order (the
 * sum every g_actions reports) for the a-bar_t that g_actions, g_pre, g_obs and g_params follow from by the VJP above, bit for
 * bit; and one wave per coefficient (the law's own adjoint) for the a-bar_t whose o-bar_t goes on into E-bar_t, so that a one-layer
 * linear policy W = G, b = 0 gives the law's g_actions, g_x0 and g_v0 bit for bit.  The two sums differ in rounding only.
 * The reverse pass is a walk, so pic_tape_backward[_feedback] and pic_tape_walk_step apply the same term at a policy step (a walk's
 * cot_modes on the field such a step read is its cot_obs and needs obs_modes == Mo, else PIC_EINVAL); pic_tape_policy_grad reads
 * the accumulated g_params after a backward or a pic_tape_walk_end (PIC_ESTATE before one, or once steps were appended).
 * pic_tape_kl_cot and pic_tape_moments_cot work unchanged on such a tape.  pic_tape_tangent* and pic_tape_tangent_walk_begin
 * return PIC_EINVAL on it: they take no parameter direction, and policy steps are never treated as open loop
 * (pic_tape_tangent_policy below is the forward-mode entry for such a tape). */
int pic_policy_vjp(pic_handle* h, const pic_policy* p, const double* obs, const double* pre, const double* cot_actions, int mem_kind,
                   double* g_params, double* g_obs, double* g_pre);
int pic_tape_step_policy(pic_handle* h, const pic_policy* p, const double* noise, const double* std, int mem_kind, int nsteps,
                         double* obs_out, double* pre_out, double* actions_out, double* hist);
int pic_tape_backward_policy(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, const double* cot_actions,
                             const double* cot_obs, int mem_kind, double* g_params, double* g_pre, double* g_obs, double* g_actions,
                             void* g_x0, void* g_v0);
int pic_tape_policy_grad(pic_handle* h, int mem_kind, double* g_params);

/* ---- Forward mode through the policy's steps (additive to ABI 5) --------------------------------------------------
 * The Jacobian-vector product of the evaluation above, for one environment, one evaluation and one direction: from the recorded
 * observation o, the recorded u (pre), a parameter tangent dtheta (per layer dW [out][in], then db [out]: the order of params),
 * an observation tangent do and an additive injection du_inj in front of the squash (the caller's d_std * eps: the library has
 * no random numbers and never sees eps).
 *   1. h_0 .. h_{L-1} are recomputed from o exactly as the forward computes them (the same bits).
 *   2. dh_0 = do, or do * obs_scale element by element.
 *   3. layer l, row i:  dy_i = db_i;  then, for k ascending, dy_i = dy_i + dW[i][k] * h_l[k];  then, for k ascending,
 *      dy_i = dy_i + W[i][k] * dh_l[k] -- every product rounded before its sum, no fused multiply-add.  With dtheta NULL
 *      dy_i starts at +0.0 and the first loop is left out (the same bits as a dtheta of zeros).
 *      Behind every layer but the last: dh_{l+1}[i] = dy_i * d_i, with d = 1.0 - h*h (tanh; h = h_{l+1}[i]) or h > 0 ? 1.0 : 0.0
 *      (relu): pic_policy_vjp's factors.
 *   4. dz = the last layer's dy;  du = dz + du_inj (du = dz without an injection).
 *   5. squash 0: da = du.  squash 1: t = tanh(u), da = (action_scale * (1.0 - t*t)) * du: pic_policy_vjp's operands.
 *      On a tape a step's d_actions is then added: da = da + d_actions.
 * Nothing is summed across lanes, workgroups or launches: K directions in one call give the bits of K calls with one each, and
 * the result does not depend on blocks_per_env, the checkpoint interval, the schedule or the batch.
 *
 * pic_policy_jvp: the JVP once for every environment and 1 <= K <= 8 directions, on obs [num_envs][2 Mo], pre [num_envs][2M]
 * (NULL allowed only with squash == 0), d_params [K][P] or [K][num_envs][P] (per_env), d_obs [K][num_envs][2 Mo], d_pre
 * [K][num_envs][2M] (each NULL = 0); d_pre_out (du) and d_actions_out (da) [K][num_envs][2M], each may be NULL.  The state is not
 * touched (allowed while a tape is open, needs no pic_reset).  Checked like pic_policy_vjp: PIC_EINVAL with the reason, nothing
 * enqueued (K outside 1..8 too).  With PIC_HOST the call waits; with PIC_DEVICE it is asynchronous.
 *
 * pic_tape_tangent_policy: pic_tape_tangent_feedback on a tape that holds steps of pic_tape_step_policy.  d_params as above is
 * the tangent of the parameters of every policy call on the tape; d_pre and d_actions [K][T][num_envs][2M] are per-step
 * injections (du_inj and the addend of item 5; rows of d_pre on other steps are ignored); d_x0 / d_v0 [K][num_envs][N]; each
 * NULL = 0.  The walk observes the policy's M_o modes: do_s = J dE_s of the field step s reads (dE_0 = K drho(x_0; dx_0)), the
 * kernel above at the taped o_s, u_s and the parameter copy of the step's call gives da_s, and de_s = B da_s drives the tangent
 * of the step as on any other.  On a mixed tape a pic_step_actions* step takes its d_actions row as its whole da_s and a gain-law
 * step da_s = G_s dm_s + d_actions_s with its taped gain (dG = 0).  Outputs, each optional: d_hist [K][T][3][num_envs], d_obs
 * [K][T][num_envs][2 Mo] (do_s), d_pre_out [K][T][num_envs][2M] (du_s, zero on other steps), d_actions_out
 * [K][T][num_envs][2M] (the da_s applied), d_x / d_v [K][num_envs][N] (final), d_E_mesh [K][T][num_envs][N_mesh].
 * Every step costs pic_tape_tangent's kernels plus the modes' one, and one more on a policy step.  The working rows, each part
 * rounded up to 256 bytes,  8 K (P or num_envs P) + 2 * 8 K (2M num_envs)  bytes, next to pic_tape_tangent_feedback's (with
 * M_o observed modes), count in pic_tape_info.bytes and against budget_bytes: PIC_ENOMEM before anything runs.  PIC_ESTATE without
 * a tape; PIC_EINVAL for K outside 1..8, a bad mem_kind or a tape without policy steps.  The call abandons a live reverse or
 * tangent walk; a replay that differs from the taped forward is reported as pic_tape_tangent reports it.  pic_tape_tangent*,
 * pic_tape_tangent_walk_begin and pic_tape_tangent_feedback keep refusing such a tape: they take no parameter direction.  A
 * tangent of the gain, d_ext, and the per-step KL's and moments' tangents are not part of this entry. */
int pic_policy_jvp(pic_handle* h, const pic_policy* p, const double* obs, const double* pre, int K, const double* d_params,
                   const double* d_obs, const double* d_pre, int mem_kind, double* d_pre_out, double* d_actions_out);
int pic_tape_tangent_policy(pic_handle* h, int K, const double* d_params, const double* d_pre, const double* d_actions,
                            const void* d_x0, const void* d_v0, int mem_kind, double* d_hist, double* d_obs, double* d_pre_out,
                            double* d_actions_out, void* d_x, void* d_v, double* d_E_mesh);

/* ---- Pooled particle features (additive to ABI 5) ------------------------------------------------------------
 * A DeepSets encoder's per-particle layer and mean, without an [N][H] array.  Per environment, with H = hidden units (1..256),
 * parameters W [H][3] row-major followed by b [H] (P = 4H float64; one vector, or [num_envs][P] with per_env, in
 * params_mem_kind memory) and a scalar v_scale, all in float64 with every product rounded before its sum (no FMA):
 *     q_i = ((2 pi) x_i) / L   (2 pi the float64 constant)      c_i, s_i = the device's cos, sin of q_i      u_i = v_i v_scale
 *     z_ik = b_k, then + W_k0 c_i, then + W_k1 s_i, then + W_k2 u_i
 *     h_ik = tanh(z_ik) (PIC_ACT_TANH) or z_ik > 0 ? z_ik : +0.0 (PIC_ACT_RELU)
 *     out_k = (sum_i h_ik) / N
 * The sum over particles is a 64-bit integer sum of the terms rounded to nearest in the unit 2^(e_k + b - 61), 2^b >= N and
 * 2^(e_k) >= B_k: B_k = 1 for tanh (e_k = 0); for relu B_k = ((|W_k0| + |W_k1|) + |W_k2| u_max) + |b_k|, times 1 + 2^-50,
 * e_k = ilogb(B_k) + 1, with u_max = max_i |u_i| of the environment, taken first as an order-independent max of bit patterns.
 * So no sum can overflow, out resolves N 2^-61 of 2^(e_k), and it depends neither on the order of the particles nor on the
 * launch geometry nor on the environment's place in the batch; two calls give the same bits.  B_k = 0 gives +0.  A non-finite
 * u_i or q_i gives NaN in every output of that environment and of no other; a non-finite W_k., b_k or B_k gives NaN in out_k.
 * pic_pool: x and v dense float64 [num_envs][N] in mem_kind memory (positions need not be wrapped), or both NULL: the handle's
 * stored particles (float64 handles only: PIC_EINVAL for float32 / fixed32; PIC_ESTATE before pic_reset and during a staged
 * step).  out [num_envs][H].  PIC_DEVICE is asynchronous on the handle's stream, PIC_HOST waits.
 * pic_pool_vjp: for a cotangent cot [num_envs][H], with a_ik = 1 - h_ik^2 (tanh) or z_ik > 0 (relu) and r_ik = (cot_k a_ik) / N,
 *     g_x_i = (2 pi / L) sum_k r_ik (W_k1 c_i - W_k0 s_i)          g_v_i = v_scale sum_k r_ik W_k2
 * (float64 sums from +0 over ascending k, one thread per particle; dense [num_envs][N] rows, overwritten) and
 *     g_W_k0 = sum_i r_ik c_i     g_W_k1 = sum_i r_ik s_i     g_W_k2 = sum_i r_ik u_i     g_b_k = sum_i r_ik
 * as integer sums in the unit of the bound (|cot_k| / N) max(1, u_max), known before the pass.  g_params is [P] -- the
 * per-environment vectors added in ascending environment order -- or [num_envs][P] with per_env; g_x, g_v, g_params may each be
 * NULL.  The activations are recomputed.  Scaling an environment's cotangent by a power of two scales its gradients bit for bit
 * while they stay normal doubles; a zero cotangent gives +0 (v_scale > 0).  The NaN rule is the forward's; a non-finite cot_k
 * gives NaN in g_W_k., g_b_k.
 * Both calls check everything before anything is enqueued (PIC_EINVAL with the reason: hidden outside 1..256, an unknown
 * activation, per_env not 0 or 1, a bad mem kind, NULL params, out or cot, exactly one of x / v NULL, a non-finite v_scale), are
 * allowed under an open tape and during a walk, and touch no particles, fields, energies, pic_bad_count, deposits or tape
 * state.  Their working memory is one block of the handle that grows to what a call needs: 8 num_envs (1 + 4H) bytes of sums and
 * max words, 8 num_envs P more for shared parameters' gradient, and the device copies of what is given in host memory. */
typedef struct pic_pool_spec {
  int32_t hidden, activation, per_env, params_mem_kind;
  double v_scale;
  const double* params;
} pic_pool_spec;
int pic_pool(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, int mem_kind, double* out);
int pic_pool_vjp(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, const double* cot, int mem_kind, void* g_x,
                 void* g_v, double* g_params);

/* ---- Pooled particle features with a LayerNorm (additive to ABI 5) ---------------------------------------------
 * The per-particle layer Linear(3, H) -> LayerNorm(H) -> activation and the mean over the particles, without an [N][H] array.
 * Parameters W [H][3] row-major, b [H], gamma [H], beta [H] (P = 6H float64; one vector, or [num_envs][P] with per_env, in
 * params_mem_kind memory), scalars v_scale, eps and period (0: the handle's L).  All arithmetic is float64 with every product
 * rounded before its sum (no FMA).  Per particle i, H = hidden units (1..256):
 *     q_i = ((2 pi) x_i) / period      c_i, s_i = the device's cos, sin of q_i      u_i = v_i v_scale      z_ik as pic_pool's
 *     mu_i = (sum_k z_ik) / H   (from +0 over ascending k)        d_ik = z_ik - mu_i
 *     var_i = (sum_k d_ik d_ik) / H   (two-pass, biased)          r_i = 1 / sqrt(var_i + eps)        y_ik = d_ik r_i
 *     n_ik = gamma_k y_ik + beta_k   (the product rounded first)
 *     h_ik = tanh(n_ik) (PIC_ACT_TANH) or n_ik > 0 ? n_ik : +0.0 (PIC_ACT_RELU)            out_k = (sum_i h_ik) / N
 * The sum over particles is pic_pool's 64-bit integer sum in the unit 2^(e_k + b - 61), 2^b >= N: e_k = 0 for tanh; for relu
 * B_k = (|gamma_k| sqrt(H) + |beta_k|) (1 + 2^-50), e_k = ilogb(B_k) + 1.  |y_ik| <= sqrt(H - 1) < sqrt(H) whatever the data, so
 * the relu unit depends on the parameters alone; B_k = 0 gives +0.  Order-free and reproducible as pic_pool.
 * pic_pool_ln_vjp: for a cotangent cot [num_envs][H], with a_ik = 1 - h_ik^2 (tanh) or n_ik > 0 (relu),
 *     dn_ik = (cot_k a_ik) / N       g_gamma_k = sum_i dn_ik y_ik       g_beta_k = sum_i dn_ik       dy_ik = dn_ik gamma_k
 *     m1_i = (sum_k dy_ik) / H       m2_i = (sum_k dy_ik y_ik) / H      dz_ik = ((dy_ik - m1_i) - y_ik m2_i) r_i
 *     g_W_k0 = sum_i dz_ik c_i    g_W_k1 = sum_i dz_ik s_i    g_W_k2 = sum_i dz_ik u_i    g_b_k = sum_i dz_ik
 *     g_x_i = (2 pi / period) sum_k dz_ik (W_k1 c_i - W_k0 s_i)         g_v_i = v_scale sum_k dz_ik W_k2
 * g_x, g_v: float64 sums from +0 over ascending k, one thread per particle; dense [num_envs][N] rows, overwritten.  The six
 * parameter sums are integer sums in the units of bounds known before the pass, each times the margin 1 + 2^-40:
 *     g_beta_k: |cot_k| / N         g_gamma_k: (|cot_k| / N) sqrt(H)
 *     g_W_k., g_b_k: ((D_k + (1 + sqrt(H)) D_max) r_max) max(1, u_max),   D_k = (|cot_k| |gamma_k|) / N,  D_max = max_k D_k,
 * r_max = max_i r_i (at most 1 / sqrt(eps)) and u_max = max_i |u_i| of the environment, both taken first as order-independent
 * maxima of bit patterns.  A zero bound gives +0, a non-finite bound NaN.  g_params is laid out as params: [P], the
 * per-environment vectors added in ascending environment order, or [num_envs][P] with per_env; g_x, g_v, g_params may each be
 * NULL.  Scaling an environment's cotangent by a power of two scales its gradients bit for bit while they stay normal doubles.
 * Non-finite and overflowing input.  An environment is NaN as a whole -- every output of that environment and of no other --
 *   - for a non-finite u_i or q_i;
 *   - for a non-finite W_k. or b_k (the mean over k spreads it to every unit);
 *   - where z or var could overflow: max_k (((|W_k0| + |W_k1|) + |W_k2| u_max) + |b_k|) > 2^500;
 *   - in pic_pool_ln_vjp also for a non-finite gamma_k, beta_k or cot_k (they reach every dz through m1, m2).
 * In pic_pool_ln a non-finite gamma_k or beta_k gives NaN in out_k alone.  The next call finds the work block clean.
 * H = 1: d = 0, y = 0, out = act(beta), and every dz is exactly +0: g_x, g_v, g_W, g_b are exactly 0.
 * Memory kinds, the stored particles (x = v = NULL; float64 handles only), state rules and refusals are pic_pool's and
 * pic_pool_vjp's, with the same messages; in addition PIC_EINVAL, before anything is enqueued, unless eps is finite and > 0 and
 * period finite and >= 0.  The working memory is pic_pool's block, laid out per call: 8 num_envs (1 + H) bytes of sums and max
 * words for pic_pool_ln, 8 num_envs (2 + 6H) for the VJP, 8 num_envs P more for shared parameters' gradient, and the device
 * copies of what is given in host memory. */
typedef struct pic_pool_ln_spec {
  int32_t hidden, activation, per_env, params_mem_kind;
  double v_scale, eps, period;
  const double* params;
} pic_pool_ln_spec;
int pic_pool_ln(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, int mem_kind, double* out);
int pic_pool_ln_vjp(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, const double* cot, int mem_kind,
                    void* g_x, void* g_v, double* g_params);

/* ---- Forward mode of the pooled particle features (additive to ABI 5) -------------------------------------------
 * pic_pool_jvp, pic_pool_ln_jvp: the directional derivatives of pic_pool / pic_pool_ln along K directions (1 <= K <= 8) in one
 * call.  d_x, d_v [K][num_envs][N] float64 in mem_kind memory, each may be NULL (0); d_params [K][P], or [K][num_envs][P] with
 * per_env, laid out as the parameters (P = 4H or 6H), in s->params_mem_kind memory, may be NULL (0); d_out [K][num_envs][H].
 * All three tangents NULL is allowed and gives +0 everywhere.  Float64, every product rounded before its sum (no FMA), the
 * additions in the order written.  With c, s, u, z, h, a_ik of the VJP and, per direction,
 *     tq_i = ((2 pi) d_x_i) / L   (period for L in the LayerNorm form)          tu_i = d_v_i v_scale
 *     dz_ik = db_k, + dW_k0 c_i, + dW_k1 s_i, + dW_k2 u_i, + (W_k1 c_i - W_k0 s_i) tq_i, + W_k2 tu_i
 * pic_pool_jvp:     d_out_k = (sum_i a_ik dz_ik) / N
 * pic_pool_ln_jvp:  dmu_i = (sum_k dz_ik) / H   (from +0 over ascending k)       e_ik = dz_ik - dmu_i
 *                   p_i = (sum_k y_ik e_ik) / H   (the same)                      dy_ik = (e_ik - y_ik p_i) r_i
 *                   dn_ik = (dgamma_k y_ik + gamma_k dy_ik) + dbeta_k             d_out_k = (sum_i a_ik dn_ik) / N
 * The sum over particles is pic_pool's 64-bit integer sum in the unit 2^(e + b - 61), 2^b >= N, 2^e above a bound on one term
 * that is known before the pass, per (direction, environment, k), each times the margin 1 + 2^-40:
 *     pic_pool_jvp:     Z_k = |db_k|, + |dW_k0|, + |dW_k1|, + |dW_k2| u_max, + (|W_k0| + |W_k1|) tq_max, + |W_k2| tu_max
 *     pic_pool_ln_jvp:  (|dgamma_k| sqrt(H) + |gamma_k| ((Z_k + (1 + sqrt(H)) Z_max) r_max)) + |dbeta_k|,   Z_max = max_k Z_k
 * (|y| <= sqrt(H), mean_k y^2 <= 1 and mean_k e^2 <= Z_max^2), with tq_max = max_i |tq_i| and tu_max = max_i |tu_i| of the
 * (direction, environment), taken in the max pass next to u_max (and r_max) as order-independent maxima of bit patterns.  So the
 * result depends neither on the order of the particles nor on the launch geometry nor on the environment's place in the batch,
 * and K directions in one call equal, bit for bit, K calls of one direction.  A zero bound deposits nothing and gives +0;
 * tangents scaled per direction by a power of two scale the result's bits by exactly that factor while everything stays a
 * normal double.
 * Non-finite input.  A non-finite u_i or q_i makes every direction of that environment NaN; a non-finite tq_i or tu_i that
 * (direction, environment) and no other.  pic_pool_jvp: a non-finite W_k., b_k, dW_k. or db_k gives NaN in d_out_k (of that
 * direction only where it is a tangent).  pic_pool_ln_jvp: whatever makes pic_pool_ln NaN as a whole does so here, and so does a
 * non-finite dW_k. or db_k for its direction (the mean over k spreads it); a non-finite gamma_k, beta_k, dgamma_k or dbeta_k
 * gives NaN in d_out_k alone.  H = 1 with the LayerNorm: every dy is +0 and the term is exactly a dbeta.  The next call of any
 * pool entry finds the work block clean.
 * x, v, the stored particles (both NULL; float64 handles only), the memory kinds, the state rules, PIC_EINVAL / PIC_ESTATE and
 * their messages are pic_pool's / pic_pool_ln's (d_out for out); in addition PIC_EINVAL, before anything is enqueued, for K
 * outside 1..8.  The working memory is pic_pool's block: 8 num_envs (1 + 2K + K H) bytes of max words and sums (one more word
 * per environment with the LayerNorm), and the device copies of what is given in host memory. */
int pic_pool_jvp(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, int K, const void* d_x, const void* d_v,
                 const double* d_params, int mem_kind, double* d_out);
int pic_pool_ln_jvp(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, int K, const void* d_x, const void* d_v,
                    const double* d_params, int mem_kind, double* d_out);

/* ---- The DeepSets particle actor in closed loop on the device (additive to ABI 5) --------------------------------
 * a = pi(x, v): the pooled particle features of pic_pool or pic_pool_ln (exactly one of `pool` / `pool_ln` is given: the
 * per-particle layer and the mean), then a head of 1..6 linear layers, with a LayerNorm and an activation behind every layer
 * but the last, evaluated by one workgroup per environment.  Float64 throughout, every product rounded before its sum (no fused
 * multiply-add).
 *   h_0 = f, the pooled features [num_envs][H]: the bits pic_pool / pic_pool_ln return for the same spec and particles.
 *   layer l: y_i = b_i; then, for k ascending, y_i = y_i + W[i][k] * h_l[k]   (pic_policy's rule).
 *   With layernorm, behind every layer but the last, over the layer's n outputs (pic_pool_ln's formulas):
 *     mu = (sum_i y_i) / n  (from +0 over ascending i)      d_i = y_i - mu      var = (sum_i d_i d_i) / n  (the same)
 *     r = 1 / sqrt(var + ln_eps)                            n_i = gamma_i (d_i r) + beta_i   (the product rounded first)
 *   Then h_{l+1} = tanh(.) (PIC_ACT_TANH) or . > 0 ? . : +0.0 (PIC_ACT_RELU) of n_i (of y_i without layernorm).
 *   z = the last layer's y.  With noise: u = z + std_i * eps_i (the product rounded first; std NULL = 1); without: u = z.
 *   squash 0: a = u.  squash 1: a = action_shift + action_scale * tanh(u)   (the product rounded first).
 * Both LayerNorm sums run over ascending i and are never split, so the result does not depend on the launch.  The library
 * draws nothing: eps is the caller's.  Non-finite input: the features follow pic_pool's / pic_pool_ln's rule (NaN in every
 * feature of an environment with a non-finite particle, and of no other); the head is plain IEEE arithmetic on them, so NaN
 * passes through linear layers, LayerNorms and tanh, while the comparison of PIC_ACT_RELU sends a NaN to +0 as pic_policy's does.
 * params: per layer W [out][in] row-major, b [out] and -- with layernorm, not behind the last layer -- gamma [out], beta [out];
 * P doubles in all, one vector or [num_envs][P] with per_env.  mem_kind covers params, features, x, v, noise, std and the three
 * outputs; the pool spec's params stay in its own params_mem_kind memory.
 *
 * pic_actor_eval: the actor once, for every environment, on one of three sources: `features` [num_envs][H] (the head alone
 * runs; the pool spec is checked but its params are not read); x and v [num_envs][N] as pic_pool takes them; or all three NULL:
 * the stored particles under pic_pool's rules (float64 handles only, after pic_reset, not inside a staged step).  noise
 * [num_envs][2M] or NULL; std [2M] or NULL.  features_out [num_envs][H], pre_out (u) and actions_out (a) [num_envs][2M]: any
 * may be NULL.  It touches no particles, fields, energies or tape state and is allowed under an open tape.
 *
 * pic_step_actor: nsteps closed-loop steps without returning to the host between them.  Step s is pic_actor_eval on the stored
 * particles step s-1 left, then the one step pic_step_actions(a_s on the device, 1) makes: the call gives the bits of the host
 * loop pic_pool[_ln](x = v = NULL) -> pic_actor_eval(features) -> pic_step_actions, on both schedules, CIC or TSC, every
 * integrator, recorder on or off.  Per step: the pool's max pass and pass, the actor's kernel (which finishes the pool's sums,
 * writes the feature row once and runs the head on it) and one step's launches; the pool call is begun once per call.  noise
 * [nsteps][num_envs][2M] or NULL; features_out [nsteps][num_envs][H]; pre_out, actions_out [nsteps][num_envs][2M]; hist: NULL,
 * or host [nsteps][3][num_envs] as pic_step_actions_traj.  Waiting: as pic_step_policy (PIC_HOST outputs or hist: one wait at
 * the end; PIC_DEVICE without hist: asynchronous on the handle's stream).
 *
 * Everything is refused before anything is enqueued, with the state untouched and the reason in pic_last_error.  PIC_EINVAL:
 * a NULL actor; both or neither of pool / pool_ln; whatever pic_pool / pic_pool_ln refuse in their spec, with their messages;
 * n_layers outside 1..6; a width outside 1..256; width[0] != hidden; width[n_layers] != 2M; layernorm, squash or per_env other
 * than 0 / 1; an unknown activation; with layernorm an ln_eps that is not finite and > 0; a non-finite action_scale or
 * action_shift; NULL params; a bad mem_kind; nsteps < 0; features together with x or v; exactly one of x / v; a handle that is
 * not float64 with float64 positions where the stored particles are read (pic_pool's message).  PIC_ESTATE: no actuator
 * (pic_set_actuator); before pic_reset or inside a staged step where the stored particles are read; pic_step_actor while a tape
 * is open (there is no taped entry: a torch policy on the tape is the route). */
typedef struct pic_actor {
  const pic_pool_spec*    pool;      /* exactly one of pool / pool_ln is non-NULL: the per-particle layer and the mean (7r / 7s) */
  const pic_pool_ln_spec* pool_ln;
  int32_t n_layers;                  /* 1..6 linear layers behind the mean */
  int32_t width[7];                  /* width[0] = the pool's hidden; width[n_layers] = 2 max_mode of pic_set_actuator; each 1..256 */
  int32_t layernorm;                 /* 0 / 1: a LayerNorm(width[l+1], ln_eps) behind every linear layer but the last */
  int32_t activation, squash, per_env;
  double  ln_eps, action_scale, action_shift;
  const double* params;              /* per layer: W [out][in] row-major, b [out], and (layernorm, not the last layer) gamma [out], beta [out] */
} pic_actor;
int pic_actor_eval(pic_handle* h, const pic_actor* a, const double* features, const void* x, const void* v, const double* noise,
                   const double* std, int mem_kind, double* features_out, double* pre_out, double* actions_out);
int pic_step_actor(pic_handle* h, const pic_actor* a, const double* noise, const double* std, int mem_kind, int nsteps,
                   double* features_out, double* pre_out, double* actions_out, double* hist);

int pic_sync(pic_handle* h);
/* Number of particle positions found non-finite or out of range by the last sweeps (0 = healthy).  Counts the state's
 * particles only: the positions of pic_eval_field / pic_compute_E probes never add to it. */
int pic_bad_count(pic_handle* h, int64_t* count);
const char* pic_last_error(pic_handle* h);   /* h may be NULL: error of the last failed pic_create */
int pic_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PICSTEP_H */
