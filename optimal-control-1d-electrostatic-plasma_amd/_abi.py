"""ctypes binding of include/picstep.h (the only way Python reaches the HIP path).

There is no CPU fallback: if libpicstep.so is missing or no HIP device is
visible, loading / creating a handle raises.
"""
import ctypes as C
import os

import numpy as np

from . import _build

PIC_F64, PIC_F32 = 0, 1
PIC_POS_FLOAT, PIC_POS_FIXED32 = 0, 1
PIC_ACC_AUTO, PIC_ACC_FIX64, PIC_ACC_PACKED, PIC_ACC_F64 = 0, 1, 2, 3
PIC_CIC, PIC_TSC = 0, 1
PIC_HOST, PIC_DEVICE = 0, 1
PIC_YOSHIDA4, PIC_SYMPLECTIC_EULER, PIC_VERLET, PIC_FORWARD_EULER = 0, 1, 2, 3
ABI_VERSION = 5

# time integrators by the reference's function names (src/env/integration.py) -> PIC_* scheme, force evaluations per step
INTEGRATORS = {"symplectic_4th_order": PIC_YOSHIDA4, "symplectic_euler": PIC_SYMPLECTIC_EULER, "verlet": PIC_VERLET,
               "forward_euler": PIC_FORWARD_EULER}
INTEGRATOR_NAMES = {v: k for k, v in INTEGRATORS.items()}
EVALS_PER_STEP = {PIC_YOSHIDA4: 3, PIC_SYMPLECTIC_EULER: 1, PIC_VERLET: 2, PIC_FORWARD_EULER: 1}


def integrator_id(integrator):
    """PIC_* scheme of `integrator`: one of the reference's function names, or a function carrying one as its __name__ (so the
    reference's own `verlet` may be passed).  Anything else raises ValueError."""
    name = integrator if isinstance(integrator, str) else getattr(integrator, "__name__", None)
    if name not in INTEGRATORS:
        raise ValueError(f"integrator must be one of {sorted(INTEGRATORS)} (a name, or a function of that name), "
                         f"not {integrator!r}")
    return INTEGRATORS[name]

# accum_dtype spellings of the Python layer -> PIC_ACC_*
ACCUMULATORS = {None: PIC_ACC_AUTO, "auto": PIC_ACC_AUTO, "fix64": PIC_ACC_FIX64, "fixed": PIC_ACC_PACKED,
                "packed": PIC_ACC_PACKED, "float64": PIC_ACC_F64}
POSITION_FORMATS = {None: PIC_POS_FLOAT, "float": PIC_POS_FLOAT, "fixed32": PIC_POS_FIXED32}

READONLY_MODES = {"auto": 0, "off": 1, "on": 2}        # pic_set_readonly_c (include/picstep.h PIC_READONLY_*)
ALTERNATE_MODES = {"auto": 0, "off": 1, "on": 2}       # pic_set_alternate_stores (PIC_ALTERNATE_*)

KIND_NAMES = ("sweep_A", "sweep_B", "sweep_C", "sweep_D", "field_solve", "sweep_aux", "resident", "sweep_integrator")


class PicConfig(C.Structure):
    _fields_ = [
        ("N", C.c_int64), ("Ng", C.c_int32), ("num_envs", C.c_int32),
        ("L", C.c_double), ("n0", C.c_double), ("dt", C.c_double), ("gamma", C.c_double),
        ("particle_dtype", C.c_int32), ("accum_dtype", C.c_int32), ("interpol", C.c_int32),
        ("device_id", C.c_int32), ("blocks_per_env", C.c_int32), ("env_index_base", C.c_int32),
        ("position_dtype", C.c_int32), ("placement", C.c_int32), ("placement_ms", C.c_int32),
    ]


class PicRecordConfig(C.Structure):
    """pic_record_config (include/picstep.h): what the rollout recorder keeps of every recorded step."""
    _fields_ = [
        ("stride", C.c_int32), ("n_modes", C.c_int32), ("x_bins", C.c_int32), ("v_bins", C.c_int32),
        ("phase_x_bins", C.c_int32), ("phase_v_bins", C.c_int32),
        ("vmin", C.c_double), ("vmax", C.c_double), ("phase_dx", C.c_double), ("phase_dv", C.c_double),
        ("feq", C.c_void_p), ("capacity", C.c_int64),
    ]


class PicRecordOut(C.Structure):
    """pic_record_out (include/picstep.h): host arrays receiving records, any may be NULL."""
    _fields_ = [(name, C.c_void_p) for name in ("step", "KE", "PE", "PE_reward", "field_energy", "entropy", "kl", "re", "im",
                                                  "x_hist", "v_hist", "inside")]


class PicTapeConfig(C.Structure):
    """pic_tape_config (include/picstep.h): capacity and checkpoint interval of a differentiable rollout."""
    _fields_ = [("max_steps", C.c_int64), ("checkpoint_every", C.c_int64), ("budget_bytes", C.c_int64)]


class PicTapeInfo(C.Structure):
    """pic_tape_info (include/picstep.h)."""
    _fields_ = [(name, C.c_int64) for name in ("steps", "checkpoint_every", "bytes", "replay_mismatches", "unit_retries",
                                                "launches", "replay_bad_positions")]


class PicPhaseSpec(C.Structure):
    """pic_phase_spec (include/picstep.h): bins, velocity range and KL target of the smoothed phase-space density."""
    _fields_ = [("nx", C.c_int32), ("nv", C.c_int32), ("vmin", C.c_double), ("vmax", C.c_double), ("feq", C.c_void_p),
                ("feq_per_env", C.c_int32), ("feq_mem_kind", C.c_int32)]


PIC_ACT_TANH, PIC_ACT_RELU = 0, 1
ACTIVATIONS = {"tanh": PIC_ACT_TANH, "relu": PIC_ACT_RELU}


class PicPolicy(C.Structure):
    """pic_policy (include/picstep.h): an MLP policy on the modes of the mesh field; params / obs_scale are addresses."""
    _fields_ = [("obs_modes", C.c_int32), ("n_layers", C.c_int32), ("width", C.c_int32 * 5), ("activation", C.c_int32),
                ("squash", C.c_int32), ("per_env", C.c_int32), ("action_scale", C.c_double), ("params", C.c_void_p),
                ("obs_scale", C.c_void_p)]


class PicPoolSpec(C.Structure):
    """pic_pool_spec (include/picstep.h): the pooled features' layer; params is an address in params_mem_kind memory."""
    _fields_ = [("hidden", C.c_int32), ("activation", C.c_int32), ("per_env", C.c_int32), ("params_mem_kind", C.c_int32),
                ("v_scale", C.c_double), ("params", C.c_void_p)]


class PicPoolLnSpec(C.Structure):
    """pic_pool_ln_spec (include/picstep.h): the layer with a LayerNorm; params (W, b, gamma, beta) is an address in
    params_mem_kind memory; period 0 = the handle's L."""
    _fields_ = [("hidden", C.c_int32), ("activation", C.c_int32), ("per_env", C.c_int32), ("params_mem_kind", C.c_int32),
                ("v_scale", C.c_double), ("eps", C.c_double), ("period", C.c_double), ("params", C.c_void_p)]


class PicActor(C.Structure):
    """pic_actor (include/picstep.h): the pooled particle features (exactly one of pool / pool_ln points to its
    spec) and a head of 1..6 linear layers; params is an address in the call's memory."""
    _fields_ = [("pool", C.POINTER(PicPoolSpec)), ("pool_ln", C.POINTER(PicPoolLnSpec)), ("n_layers", C.c_int32),
                ("width", C.c_int32 * 7), ("layernorm", C.c_int32), ("activation", C.c_int32), ("squash", C.c_int32),
                ("per_env", C.c_int32), ("ln_eps", C.c_double), ("action_scale", C.c_double), ("action_shift", C.c_double),
                ("params", C.c_void_p)]


class PicError(RuntimeError):
    pass


_lib = None

# name -> argtypes; every entry point of include/picstep.h is listed (tests check the exports)
_vp, _dp, _i64p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)
SIGNATURES = {
    "pic_create": [C.POINTER(PicConfig), C.POINTER(_vp)],
    "pic_destroy": [_vp],
    "pic_reset": [_vp, _vp, _vp, C.c_int],
    "pic_reset_sampled": [_vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64],
    "pic_step": [_vp, _vp, C.c_int, C.c_int],
    "pic_step_stage": [_vp, C.c_int, _vp, C.c_int],
    "pic_set_integrator": [_vp, C.c_int],
    "pic_set_readonly_c": [_vp, C.c_int],
    "pic_set_alternate_stores": [_vp, C.c_int],
    "pic_get_integrator": [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "pic_step_history": [_vp, _vp, C.c_int, C.c_int, _vp],
    "pic_step_snapshots": [_vp, _vp, C.c_int, C.c_int, _vp, _vp],
    "pic_get_particles": [_vp, _vp, _vp, C.c_int],
    "pic_set_particles": [_vp, _vp, _vp, C.c_int],
    "pic_refresh": [_vp],
    "pic_invalidate": [_vp],
    "pic_device_ptrs": [_vp] + [C.POINTER(_vp)] * 2 + [_i64p] + [C.POINTER(_vp)] * 6,
    "pic_get_fields": [_vp, _vp, _vp, _vp],
    "pic_get_energies": [_vp, _vp, _vp, _vp],
    "pic_gather_E": [_vp, _vp, C.c_int],
    "pic_get_cic": [_vp, C.c_int, _vp, _vp, _vp, _vp],
    "pic_eval_field": [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp],
    "pic_compute_E": [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pic_solve_poisson": [_vp, _vp, _vp, _vp],
    "pic_profile": [_vp, C.c_int],
    "pic_profile_read": [_vp, _dp, _i64p],
    "pic_set_actuator": [_vp, C.c_int, _vp, _vp],
    "pic_step_actions": [_vp, _vp, C.c_int, C.c_int],
    "pic_step_actions_traj": [_vp, _vp, C.c_int, C.c_int, _vp],
    "pic_step_ext_traj": [_vp, _vp, C.c_int, C.c_int, _vp, _vp],
    "pic_step_feedback": [_vp, C.c_int, C.c_int, _vp, _vp],
    "pic_step_feedback_gain": [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp],
    "pic_step_observe": [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp],
    "pic_get_modes": [_vp, C.c_int, _vp, _vp, C.c_int],
    "pic_phase_histogram": [_vp, C.c_int, C.c_double, C.c_double, _vp],
    "pic_phase_kl": [_vp, C.c_int, C.c_double, C.c_double, _vp, _vp],
    "pic_phase_kl_smooth": [_vp, C.POINTER(PicPhaseSpec), C.c_int, _vp, _vp],
    "pic_phase_kl_smooth_vjp": [_vp, C.POINTER(PicPhaseSpec), _vp, C.c_int, _vp, _vp],
    "pic_phase_kl_smooth_jvp": [_vp, C.POINTER(PicPhaseSpec), C.c_int, _vp, _vp, C.c_int, _vp],
    "pic_stream_probe": [_vp, C.c_int, _dp],
    "pic_record_start": [_vp, C.POINTER(PicRecordConfig)],
    "pic_record_now": [_vp],
    "pic_record_count": [_vp, _i64p],
    "pic_record_read": [_vp, C.c_int64, C.c_int64, C.POINTER(PicRecordOut)],
    "pic_record_stop": [_vp],
    "pic_tape_start": [_vp, C.POINTER(PicTapeConfig)],
    "pic_tape_backward": [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp],
    "pic_tape_backward_feedback": [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp],
    "pic_tape_stats": [_vp, C.POINTER(PicTapeInfo)],
    "pic_tape_stop": [_vp],
    "pic_tape_walk_begin": [_vp, C.c_int, C.c_int],
    "pic_tape_walk_step": [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _i64p],
    "pic_tape_walk_end": [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp],
    "pic_tape_tangent": [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp],
    "pic_tape_tangent_kl": [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp],
    "pic_tape_kl_start": [_vp, C.POINTER(PicPhaseSpec)],
    "pic_tape_kl": [_vp, C.c_int, _vp],
    "pic_tape_kl_cot": [_vp, _vp, C.c_int, C.c_int64, C.c_int64],
    "pic_moments": [_vp, C.c_int, _vp],
    "pic_moments_vjp": [_vp, _vp, C.c_int, _vp, _vp],
    "pic_tape_moments_cot": [_vp, _vp, C.c_int, C.c_int64, C.c_int64],
    "pic_moments_jvp": [_vp, C.c_int, _vp, _vp, C.c_int, _vp],
    "pic_tape_moments_start": [_vp],
    "pic_tape_moments": [_vp, C.c_int, _vp],
    "pic_tape_tangent_moments": [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "pic_tape_tangent_walk_begin": [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp],
    "pic_tape_tangent_walk_step": [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64p],
    "pic_tape_tangent_walk_end": [_vp, C.c_int, _vp, _vp],
    "pic_tape_tangent_feedback": [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "pic_set_stream": [_vp, _vp],
    "pic_own_stream": [_vp],
    "pic_schedule": [_vp],
    "pic_placement_info": [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "pic_placement_stats": [_vp, _vp],
    "pic_copy_envs": [_vp, _vp, _vp, C.c_int],
    "pic_copy_envs_rejected": [_vp, _i64p],
    "pic_policy_eval": [_vp, C.POINTER(PicPolicy), _vp, _vp, _vp, C.c_int, _vp, _vp, _vp],
    "pic_step_policy": [_vp, C.POINTER(PicPolicy), _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "pic_policy_vjp": [_vp, C.POINTER(PicPolicy), _vp, _vp, _vp, C.c_int, _vp, _vp, _vp],
    "pic_tape_step_policy": [_vp, C.POINTER(PicPolicy), _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "pic_tape_backward_policy": [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "pic_tape_policy_grad": [_vp, C.c_int, _vp],
    "pic_policy_jvp": [_vp, C.POINTER(PicPolicy), _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp],
    "pic_tape_tangent_policy": [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pic_pool": [_vp, C.POINTER(PicPoolSpec), _vp, _vp, C.c_int, _vp],
    "pic_pool_vjp": [_vp, C.POINTER(PicPoolSpec), _vp, _vp, _vp, C.c_int, _vp, _vp, _vp],
    "pic_pool_ln": [_vp, C.POINTER(PicPoolLnSpec), _vp, _vp, C.c_int, _vp],
    "pic_pool_ln_vjp": [_vp, C.POINTER(PicPoolLnSpec), _vp, _vp, _vp, C.c_int, _vp, _vp, _vp],
    "pic_pool_jvp": [_vp, C.POINTER(PicPoolSpec), _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp],
    "pic_pool_ln_jvp": [_vp, C.POINTER(PicPoolLnSpec), _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp],
    "pic_actor_eval": [_vp, C.POINTER(PicActor), _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp],
    "pic_step_actor": [_vp, C.POINTER(PicActor), _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "pic_sync": [_vp],
    "pic_bad_count": [_vp, _i64p],
    "pic_last_error": [_vp],
    "pic_abi_version": [],
}


class _Placement(C.Structure):
    _fields_ = [("pairs_timed", C.c_int32), ("blocks", C.c_int32), ("outcome", C.c_int32), ("legs", C.c_int32),
                ("kept_gbytes_per_s", C.c_double), ("slowest_gbytes_per_s", C.c_double), ("seconds", C.c_double),
                ("malloc_seconds", C.c_double), ("timing_seconds", C.c_double), ("free_seconds", C.c_double)]


def library_path():
    """The one library this package loads: csrc/libpicstep.so next to it (no environment override)."""
    return _build.LIB


def _preload_torch_hip_runtime():
    """One HIP runtime per process: the torch wheel bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7, the name libpicstep.so needs).  Loading that copy first makes the dynamic
    loader bind libpicstep.so to it, so torch tensors and library buffers share one runtime,
    whichever of the two is imported first.  Without torch the system ROCm runtime is used."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    """Load csrc/libpicstep.so (built by __graft_entry__.build()); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path) and path == _build.LIB:
        try:                                   # a checkout without the built library: compile it now (hipcc, gfx950)
            _build.build_library()
        except RuntimeError as e:
            raise PicError(f"{path} is missing and could not be built ({e}). There is no CPU fallback for the "
                           "PIC step.") from e
    if not os.path.exists(path):
        raise PicError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc, gfx950). There is no CPU fallback for the PIC step.")
    _preload_torch_hip_runtime()
    lib = C.CDLL(path)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_char_p if name == "pic_last_error" else C.c_int
    if lib.pic_abi_version() != ABI_VERSION:
        raise PicError("libpicstep.so ABI version mismatch: rebuild it")
    _lib = lib
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    # (ndarray.ctypes costs ~1.5 us per use and a Gym iteration passes nine pointers.  The bare address keeps no reference to
    # the array: every caller passes a name, or a view of one, that outlives the call)
    return C.c_void_p(a.__array_interface__["data"][0])


def _ptrs(*addresses):
    """Addresses (int, 0 or None = NULL) as pointer arguments."""
    return [_ptr(int(q)) if q else None for q in addresses]


def _host(a, shape):
    """a (or None) as a C-contiguous float64 host array of `shape`."""
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))


def _addrs(*arrays):
    """The addresses of host arrays (None -> 0), for the entry points that take addresses and a mem_kind."""
    return [0 if a is None else a.__array_interface__["data"][0] for a in arrays]


def _phase_spec(nx, nv, vmin, vmax, feq, feq_per_env, feq_kind):
    """pic_phase_spec; feq an address (0 = NULL) in feq_kind memory."""
    return PicPhaseSpec(int(nx), int(nv), float(vmin), float(vmax), int(feq) or None, int(feq_per_env), int(feq_kind))


class Handle:
    """Owns one pic_handle (one device, one stream, `num_envs` environments)."""

    def __init__(self, N, Ng, num_envs=1, L=50.0, n0=1.0, dt=0.1, gamma=5.0, particle_dtype="float64",
                 accum_dtype=None, interpol="CIC", device_id=0, blocks_per_env=0, env_index_base=0,
                 position_dtype=None, placement="auto", placement_ms=0, integrator="symplectic_4th_order", readonly_c="auto",
                 alternate_stores="auto"):
        scheme = integrator_id(integrator)
        if alternate_stores not in ALTERNATE_MODES:
            raise ValueError(f"alternate_stores must be one of {sorted(ALTERNATE_MODES)}, not {alternate_stores!r}")
        if readonly_c not in READONLY_MODES:
            raise ValueError(f"readonly_c must be one of {sorted(READONLY_MODES)}, not {readonly_c!r}")
        self.lib = load()
        pd = {"float64": PIC_F64, "float32": PIC_F32}[str(np.dtype(particle_dtype))]
        # LDS mesh accumulator (include/picstep.h PIC_ACC_*).  None: the library's choice -- the packed word for
        # float32 CIC (one integer LDS atomic per deposit), 64-bit fixed point otherwise; both are integer sums, so
        # a step is bitwise reproducible.  "float64" = float64 running sums (ds_add_f64), float64 particles only.
        key = accum_dtype if accum_dtype is None else str(accum_dtype)
        if key not in ACCUMULATORS:
            raise ValueError(f"accum_dtype must be one of {sorted(k for k in ACCUMULATORS if k)} or None, not {accum_dtype!r}")
        pkey = position_dtype if position_dtype is None else str(position_dtype)
        if pkey not in POSITION_FORMATS:
            raise ValueError(f"position_dtype must be 'float', 'fixed32' or None, not {position_dtype!r}")
        self.cfg = PicConfig(int(N), int(Ng), int(num_envs), float(L), float(n0), float(dt), float(gamma), pd,
                             ACCUMULATORS[key], {"CIC": PIC_CIC, "TSC": PIC_TSC}[interpol], int(device_id),
                             int(blocks_per_env), int(env_index_base), POSITION_FORMATS[pkey],
                             {"auto": 0, "off": 1}[placement], int(placement_ms))
        self.fixed_positions = POSITION_FORMATS[pkey] == PIC_POS_FIXED32
        self.N, self.Ng, self.num_envs = int(N), int(Ng), int(num_envs)
        self.dtype = np.dtype(particle_dtype)
        self.max_mode = 0                              # (no actuator yet: set_actuator)
        self._taping, self._law_calls = False, []      # (first step, steps) of every gain-law call on the open tape
        self._h = C.c_void_p()
        rc = self.lib.pic_create(C.byref(self.cfg), C.byref(self._h))
        if rc != 0:
            msg = self.lib.pic_last_error(None)
            self._h = C.c_void_p()
            raise PicError(f"pic_create failed ({rc}): {msg.decode() if msg else ''}")
        if scheme != PIC_YOSHIDA4:
            self.set_integrator(scheme)
        if readonly_c != "auto":
            self.set_readonly_c(readonly_c)
        if alternate_stores != "auto":
            self.set_alternate_stores(alternate_stores)

    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.pic_last_error(self._h)
            raise PicError(f"libpicstep error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.pic_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state -------------------------------------------------------------------------------
    def _particles_in(self, a):
        a = np.ascontiguousarray(np.asarray(a, dtype=self.dtype).reshape(self.num_envs, self.N))
        return a

    def reset(self, x0, v0):
        x0, v0 = self._particles_in(x0), self._particles_in(v0)
        self._chk(self.lib.pic_reset(self._h, _ptr(x0), _ptr(v0), PIC_HOST))

    def reset_device(self, x_ptr, v_ptr):
        self._chk(self.lib.pic_reset(self._h, _ptr(int(x_ptr)), _ptr(int(v_ptr)), PIC_DEVICE))

    def reset_sampled(self, kind, a=0.2, v0=3.0, sigma=1.0, A=0.1, n_mode=2, seed=0):
        k = {"two-stream": 0, "bump-on-tail": 1}[kind]
        self._chk(self.lib.pic_reset_sampled(self._h, k, float(a), float(v0), float(sigma), float(A), int(n_mode),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_particles(self, x, v):
        x, v = self._particles_in(x), self._particles_in(v)
        self._chk(self.lib.pic_set_particles(self._h, _ptr(x), _ptr(v), PIC_HOST))

    def refresh(self):
        self._chk(self.lib.pic_refresh(self._h))

    def invalidate(self):
        """Call after writing x / v through the device views (or call refresh())."""
        self._chk(self.lib.pic_invalidate(self._h))

    def copy_envs(self, src, map=None):
        """pic_copy_envs: environment e of this handle becomes environment map[e] of `src` (a Handle; this one: a fork).  map: a
        sequence or NumPy array of num_envs indices (checked on the host), an int32 CUDA tensor of that length (passed by
        pointer and checked by the kernels: copy_envs_rejected), or None (two handles of equal num_envs: the identity).
        Asynchronous on this handle's stream."""
        if map is None:
            ptr, kind = None, PIC_HOST
        elif hasattr(map, "data_ptr"):
            if not (map.is_cuda and map.element_size() == 4 and not map.dtype.is_floating_point and map.is_contiguous()
                    and tuple(map.shape) == (self.num_envs,)):
                raise ValueError("map must be a contiguous int32 CUDA tensor [num_envs]")
            ptr, kind = _ptr(int(map.data_ptr())), PIC_DEVICE
        else:
            m = np.asarray(map)
            if m.shape != (self.num_envs,) or m.dtype.kind not in "iu":
                raise ValueError(f"map must hold num_envs = {self.num_envs} integer indices")
            m = np.ascontiguousarray(np.clip(m, -1, 2 ** 31 - 1), dtype=np.int32)      # (out of int32's range: refused as -1 / too large)
            ptr, kind = _ptr(m), PIC_HOST
        self._chk(self.lib.pic_copy_envs(self._h, src._h, ptr, kind))

    def copy_envs_rejected(self):
        """Entries of device maps that copy_envs' kernels refused since the handle was created (waits for the stream)."""
        c = C.c_int64()
        self._chk(self.lib.pic_copy_envs_rejected(self._h, C.byref(c)))
        return c.value

    def set_alternate_stores(self, mode):
        """pic_set_alternate_stores: "auto", "off" or "on" -- whether every second inner step of a call stores once (same bits)."""
        self._chk(self.lib.pic_set_alternate_stores(self._h, ALTERNATE_MODES[mode]))

    def set_readonly_c(self, mode):
        """pic_set_readonly_c: "auto", "off" or "on" -- whether whole steps leave sweep C's stores to sweep D (same bits)."""
        self._chk(self.lib.pic_set_readonly_c(self._h, READONLY_MODES[mode]))

    def set_integrator(self, integrator):
        """Time integrator of the later steps: a PIC_* scheme, a reference function name or a function of that name."""
        scheme = integrator if isinstance(integrator, int) else integrator_id(integrator)
        self._chk(self.lib.pic_set_integrator(self._h, int(scheme)))

    def integrator(self):
        """-> (reference function name, force evaluations per step)"""
        scheme, evals = C.c_int(), C.c_int()
        self._chk(self.lib.pic_get_integrator(self._h, C.byref(scheme), C.byref(evals)))
        return INTEGRATOR_NAMES[scheme.value], evals.value

    def step(self, E_ext=None, nsteps=1):
        if E_ext is None:
            self._chk(self.lib.pic_step(self._h, None, PIC_HOST, int(nsteps)))
        else:
            e = np.ascontiguousarray(np.asarray(E_ext, dtype=np.float64).reshape(self.num_envs, self.Ng))
            self._chk(self.lib.pic_step(self._h, _ptr(e), PIC_HOST, int(nsteps)))

    def step_device(self, E_ext_ptr, nsteps=1):
        self._chk(self.lib.pic_step(self._h, _ptr(int(E_ext_ptr)) if E_ext_ptr else None, PIC_DEVICE, int(nsteps)))

    def sync(self):
        self._chk(self.lib.pic_sync(self._h))

    def schedule(self):
        """'resident' (one launch per pic_step call, small environments) or 'streaming' (sweeps)."""
        return "resident" if self.lib.pic_schedule(self._h) == 1 else "streaming"

    def placement_info(self):
        """((x, v) placements pic_create timed, GB/s of the pair kept, GB/s of the slowest pair, seconds the search took);
        (1, 0, 0, 0) for small states and with placement="off"."""
        n, kept, slow, sec = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.pic_placement_info(self._h, C.byref(n), C.byref(kept), C.byref(slow), C.byref(sec)))
        return n.value, kept.value, slow.value, sec.value

    def placement_stats(self):
        """pic_placement_stats as a dict: pairs_timed, blocks, legs, outcome ("none" | "found" | "patience" | "timeout" | "memory"),
        kept_GBs, slowest_GBs, seconds, malloc_seconds, timing_seconds, free_seconds."""
        st = _Placement()
        self._chk(self.lib.pic_placement_stats(self._h, C.byref(st)))
        return {"pairs_timed": st.pairs_timed, "blocks": st.blocks, "legs": st.legs,
                "outcome": ("none", "found", "patience", "timeout", "memory")[st.outcome], "kept_GBs": st.kept_gbytes_per_s,
                "slowest_GBs": st.slowest_gbytes_per_s, "seconds": st.seconds, "malloc_seconds": st.malloc_seconds,
                "timing_seconds": st.timing_seconds, "free_seconds": st.free_seconds}

    def particles(self):
        x = np.empty((self.num_envs, self.N), dtype=self.dtype)
        v = np.empty_like(x)
        self._chk(self.lib.pic_get_particles(self._h, _ptr(x), _ptr(v), PIC_HOST))
        return x, v

    def fields(self):
        n = np.empty((self.num_envs, self.Ng))
        E = np.empty_like(n)
        phi = np.empty_like(n)
        self._chk(self.lib.pic_get_fields(self._h, _ptr(n), _ptr(E), _ptr(phi)))
        return n, E, phi

    def energies(self):
        ke = np.empty(self.num_envs)
        pe = np.empty_like(ke)
        per = np.empty_like(ke)
        self._chk(self.lib.pic_get_energies(self._h, _ptr(ke), _ptr(pe), _ptr(per)))
        return ke, pe, per

    def gather_E(self):
        E = np.empty((self.num_envs, self.N), dtype=self.dtype)
        self._chk(self.lib.pic_gather_E(self._h, _ptr(E), PIC_HOST))
        return E

    def cic(self, env=0):
        jl = np.empty(self.N, dtype=np.int64)
        jr = np.empty_like(jl)
        wl = np.empty(self.N)
        wr = np.empty_like(wl)
        self._chk(self.lib.pic_get_cic(self._h, int(env), _ptr(jl), _ptr(jr), _ptr(wl), _ptr(wr)))
        return jl, jr, wl, wr

    def eval_field(self, x, E_ext=None, fields=True):
        """compute_E on arbitrary positions -> (n, E_mesh(+E_ext), 0.5*sum(E^2)*dx) per env (n, E_mesh None with fields=False:
        a caller that wants the energy alone saves two read-backs)."""
        x = self._particles_in(x)
        e = None if E_ext is None else np.ascontiguousarray(np.asarray(E_ext, dtype=np.float64).reshape(self.num_envs, self.Ng))
        n = np.empty((self.num_envs, self.Ng)) if fields else None
        E = np.empty_like(n) if fields else None
        pe = np.empty(self.num_envs)
        self._chk(self.lib.pic_eval_field(self._h, _ptr(x), PIC_HOST, _ptr(e), _ptr(n), _ptr(E), _ptr(pe)))
        return n, E, pe

    def step_stage(self, stage, E_ext=None):
        e = None if E_ext is None else np.ascontiguousarray(np.asarray(E_ext, dtype=np.float64).reshape(self.num_envs, self.Ng))
        self._chk(self.lib.pic_step_stage(self._h, int(stage), _ptr(e), PIC_HOST))

    def step_history(self, E_ext=None, nsteps=1):
        """nsteps steps; returns (KE, PE, PE_reward), each [nsteps][num_envs], the energies after every step."""
        e = None if E_ext is None else np.ascontiguousarray(np.asarray(E_ext, dtype=np.float64).reshape(self.num_envs, self.Ng))
        hist = np.empty((int(nsteps), 3, self.num_envs))
        self._chk(self.lib.pic_step_history(self._h, _ptr(e), PIC_HOST, int(nsteps), _ptr(hist)))
        return hist[:, 0], hist[:, 1], hist[:, 2]

    def step_snapshots(self, E_ext=None, nsteps=1):
        """nsteps steps; returns (x, v, KE, PE, PE_reward): particles after every step [nsteps][num_envs][N] and the
        energies [nsteps][num_envs] -- what PIC.simulate records, with one read-back at the end."""
        e = None if E_ext is None else np.ascontiguousarray(np.asarray(E_ext, dtype=np.float64).reshape(self.num_envs, self.Ng))
        snap = np.empty((int(nsteps), 2, self.num_envs, self.N), dtype=self.dtype)
        hist = np.empty((int(nsteps), 3, self.num_envs))
        self._chk(self.lib.pic_step_snapshots(self._h, _ptr(e), PIC_HOST, int(nsteps), _ptr(snap), _ptr(hist)))
        return snap[:, 0], snap[:, 1], hist[:, 0], hist[:, 1], hist[:, 2]

    def compute_E(self, x, E_ext=None, particles=True, shape=False):
        """compute_E(return_all=True) + shape bookkeeping on arbitrary positions.  Returns a dict with
        n, E_mesh (incl. E_ext), phi_mesh [env][Ng]; E, phi [env][N] if `particles`; idx (int64), w [env][3][N]
        if `shape` (rows l, r, - for CIC; l, m, r for TSC)."""
        x = self._particles_in(x)
        E_, N, Ng = self.num_envs, self.N, self.Ng
        e = None if E_ext is None else np.ascontiguousarray(np.asarray(E_ext, dtype=np.float64).reshape(E_, Ng))
        out = {"n": np.empty((E_, Ng)), "E_mesh": np.empty((E_, Ng)), "phi_mesh": np.empty((E_, Ng))}
        if particles:
            out["E"] = np.empty((E_, N), dtype=self.dtype)
            out["phi"] = np.empty((E_, N), dtype=self.dtype)
        if shape:
            out["idx"] = np.empty((E_, 3, N), dtype=np.int64)
            out["w"] = np.empty((E_, 3, N))
        self._chk(self.lib.pic_compute_E(self._h, _ptr(x), PIC_HOST, _ptr(e), _ptr(out.get("E")), _ptr(out.get("phi")),
                                         _ptr(out["n"]), _ptr(out["E_mesh"]), _ptr(out["phi_mesh"]),
                                         _ptr(out.get("idx")), _ptr(out.get("w"))))
        return out

    def solve_poisson(self, rhs):
        """Periodic 3-point Poisson solve of rhs [env][Ng] (zero sum) -> (phi with zero mean, E_mesh = -grad phi)."""
        b = np.ascontiguousarray(np.asarray(rhs, dtype=np.float64).reshape(self.num_envs, self.Ng))
        phi = np.empty_like(b)
        E = np.empty_like(b)
        self._chk(self.lib.pic_solve_poisson(self._h, _ptr(b), _ptr(phi), _ptr(E)))
        return phi, E

    def device_ptrs(self):
        ps = [C.c_void_p() for _ in range(8)]
        ld = C.c_int64()
        self._chk(self.lib.pic_device_ptrs(self._h, C.byref(ps[0]), C.byref(ps[1]), C.byref(ld), C.byref(ps[2]),
                                           C.byref(ps[3]), C.byref(ps[4]), C.byref(ps[5]), C.byref(ps[6]),
                                           C.byref(ps[7])))
        names = ("x", "v", "n", "E_mesh", "phi", "KE", "PE", "PE_reward")
        out = {k: p.value for k, p in zip(names, ps)}
        out["ld"] = ld.value
        return out

    def profile(self, enable=True):
        self._chk(self.lib.pic_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        ms = (C.c_double * 8)()
        cnt = (C.c_int64 * 8)()
        self._chk(self.lib.pic_profile_read(self._h, ms, cnt))
        return {KIND_NAMES[i]: (ms[i], cnt[i]) for i in range(8) if cnt[i]}

    def set_actuator(self, basis_cos, basis_sin):
        bc = np.ascontiguousarray(basis_cos, dtype=np.float64)
        bs = np.ascontiguousarray(basis_sin, dtype=np.float64)
        if bc.shape != bs.shape or bc.shape[0] != self.Ng:
            raise ValueError("basis tables must be [Ng, max_mode]")
        self.max_mode = int(bc.shape[1])
        self._chk(self.lib.pic_set_actuator(self._h, self.max_mode, _ptr(bc), _ptr(bs)))

    def step_actions(self, actions, nsteps=1):
        a = np.ascontiguousarray(np.asarray(actions, dtype=np.float64).reshape(self.num_envs, 2 * self.max_mode))
        self._chk(self.lib.pic_step_actions(self._h, _ptr(a), PIC_HOST, int(nsteps)))

    def step_actions_device(self, actions_ptr, nsteps=1):
        self._chk(self.lib.pic_step_actions(self._h, _ptr(int(actions_ptr)), PIC_DEVICE, int(nsteps)))

    def _hist_out(self, nsteps, history):
        return np.empty((int(nsteps), 3, self.num_envs)) if history else None

    def step_actions_traj(self, actions, history=False):
        """One step per row of actions [nsteps][num_envs][2*max_mode], all in one call (pic_step_actions_traj).
        history=True: returns (KE, PE, PE_reward), each [nsteps][num_envs]; otherwise asynchronous, returns None."""
        a = np.ascontiguousarray(np.asarray(actions, dtype=np.float64))
        a = a.reshape(-1, self.num_envs, 2 * self.max_mode)
        hist = self._hist_out(a.shape[0], history)
        self._chk(self.lib.pic_step_actions_traj(self._h, _ptr(a), PIC_HOST, a.shape[0], _ptr(hist)))
        return None if hist is None else (hist[:, 0], hist[:, 1], hist[:, 2])

    def step_actions_traj_device(self, actions_ptr, nsteps):
        """actions: device pointer to [nsteps][num_envs][2*max_mode] float64; asynchronous on the handle's stream."""
        self._chk(self.lib.pic_step_actions_traj(self._h, _ptr(int(actions_ptr)), PIC_DEVICE, int(nsteps), None))

    def step_ext_traj(self, E_ext_traj, history=False, snapshots=False):
        """One step per row of E_ext_traj [nsteps][num_envs][Ng] (pic_step_ext_traj): PIC.simulate(E_external_traj).
        Returns None, (KE, PE, PE_reward), or (x, v, KE, PE, PE_reward) with snapshots=True."""
        e = np.ascontiguousarray(np.asarray(E_ext_traj, dtype=np.float64)).reshape(-1, self.num_envs, self.Ng)
        k = e.shape[0]
        hist = self._hist_out(k, history or snapshots)
        snap = np.empty((k, 2, self.num_envs, self.N), dtype=self.dtype) if snapshots else None
        self._chk(self.lib.pic_step_ext_traj(self._h, _ptr(e), PIC_HOST, k, _ptr(hist), _ptr(snap)))
        if snapshots:
            return snap[:, 0], snap[:, 1], hist[:, 0], hist[:, 1], hist[:, 2]
        return None if hist is None else (hist[:, 0], hist[:, 1], hist[:, 2])

    def step_feedback(self, nsteps, actions=False, history=False):
        """nsteps of the linear feedback loop on the device (pic_step_feedback; the actuator's max_mode).  Returns a dict with
        "actions" [nsteps][num_envs][2*max_mode] and / or "KE", "PE", "PE_reward" [nsteps][num_envs] as asked for; with
        neither the call is asynchronous and returns None."""
        k = int(nsteps)
        act = np.empty((k, self.num_envs, 2 * self.max_mode)) if actions else None
        hist = self._hist_out(k, history)
        self._chk(self.lib.pic_step_feedback(self._h, self.max_mode, k, _ptr(act), _ptr(hist)))
        out = {}
        if act is not None:
            out["actions"] = act
        if hist is not None:
            out.update(KE=hist[:, 0], PE=hist[:, 1], PE_reward=hist[:, 2])
        return out or None

    def step_feedback_gain(self, gain, nsteps, actions=False, modes=False, history=False, device_ptr=None):
        """nsteps of the gain law a = G m on the device (pic_step_feedback_gain; the actuator's max_mode).  gain: host
        [num_envs][2M][2M] float64, or device_ptr (an address of such an array on the device; gain is then ignored).  Returns a
        dict with "actions", "modes" [nsteps][num_envs][2M] and / or "KE", "PE", "PE_reward" [nsteps][num_envs] as asked for;
        with none of them the call is asynchronous and returns None."""
        k = int(nsteps)
        E, n = self.num_envs, 2 * self.max_mode
        if device_ptr is None:
            g = np.ascontiguousarray(np.asarray(gain, dtype=np.float64))
            if g.shape != (E, n, n):
                raise ValueError(f"gain must be [num_envs, 2*max_mode, 2*max_mode] = {(E, n, n)}, got {g.shape}")
            gp, kind = _ptr(g), PIC_HOST
        else:
            gp, kind = _ptr(int(device_ptr)), PIC_DEVICE
        act = np.empty((k, E, n)) if actions else None
        md = np.empty((k, E, n)) if modes else None
        hist = self._hist_out(k, history)
        first = self.tape_stats()["steps"] if self._taping else None
        self._chk(self.lib.pic_step_feedback_gain(self._h, self.max_mode, gp, kind, k, _ptr(act), _ptr(md), _ptr(hist)))
        if first is not None and k > 0:
            self._law_calls.append((first, k))
        out = {}
        if act is not None:
            out["actions"] = act
        if md is not None:
            out["modes"] = md
        if hist is not None:
            out.update(KE=hist[:, 0], PE=hist[:, 1], PE_reward=hist[:, 2])
        return out or None

    def policy_eval(self, spec, obs, noise, std, kind, obs_out, pre_out, actions_out):
        """pic_policy_eval on addresses (0 or None = NULL) in `kind` memory; spec: a PicPolicy whose params / obs_scale are
        addresses in the same memory."""
        self._chk(self.lib.pic_policy_eval(self._h, C.byref(spec), *_ptrs(obs, noise, std), int(kind),
                                           *_ptrs(obs_out, pre_out, actions_out)))

    def step_policy(self, spec, noise, std, kind, nsteps, obs_out, pre_out, actions_out, hist=None):
        """pic_step_policy on addresses (0 or None = NULL) in `kind` memory; hist: a host array [nsteps][3][num_envs] or None."""
        self._chk(self.lib.pic_step_policy(self._h, C.byref(spec), *_ptrs(noise, std), int(kind), int(nsteps),
                                           *_ptrs(obs_out, pre_out, actions_out), _ptr(hist)))

    # -- the DeepSets particle actor in closed loop ---------------------------------------------------------------
    def actor_eval(self, spec, features, x, v, noise, std, kind, features_out, pre_out, actions_out):
        """pic_actor_eval on addresses (0 or None = NULL) in `kind` memory; spec: a PicActor whose params is an address in the
        same memory and whose pool / pool_ln points to a live spec."""
        self._chk(self.lib.pic_actor_eval(self._h, C.byref(spec), *_ptrs(features, x, v, noise, std), int(kind),
                                          *_ptrs(features_out, pre_out, actions_out)))

    def step_actor(self, spec, noise, std, kind, nsteps, features_out, pre_out, actions_out, hist=None):
        """pic_step_actor on addresses (0 or None = NULL) in `kind` memory; hist: a host array [nsteps][3][num_envs] or None."""
        self._chk(self.lib.pic_step_actor(self._h, C.byref(spec), *_ptrs(noise, std), int(kind), int(nsteps),
                                          *_ptrs(features_out, pre_out, actions_out), _ptr(hist)))

    # -- policy gradients on the device -------------------------------------------------------------------------
    def policy_vjp(self, spec, obs, pre, cot_actions, kind, g_params, g_obs, g_pre):
        """pic_policy_vjp on addresses (0 or None = NULL) in `kind` memory; spec as for policy_eval."""
        self._chk(self.lib.pic_policy_vjp(self._h, C.byref(spec), *_ptrs(obs, pre, cot_actions), int(kind),
                                          *_ptrs(g_params, g_obs, g_pre)))

    def tape_step_policy(self, spec, noise, std, kind, nsteps, obs_out, pre_out, actions_out, hist=None):
        """pic_tape_step_policy: step_policy's arguments, on an open tape."""
        self._chk(self.lib.pic_tape_step_policy(self._h, C.byref(spec), *_ptrs(noise, std), int(kind), int(nsteps),
                                                *_ptrs(obs_out, pre_out, actions_out), _ptr(hist)))

    def tape_backward_policy(self, kind, cot_hist, cot_x, cot_v, cot_actions, cot_obs, g_params, g_pre, g_obs, g_actions, g_x0, g_v0):
        """pic_tape_backward_policy on addresses (0 or None = NULL) in `kind` memory."""
        p = _ptrs(cot_hist, cot_x, cot_v, cot_actions, cot_obs, g_params, g_pre, g_obs, g_actions, g_x0, g_v0)
        self._chk(self.lib.pic_tape_backward_policy(self._h, *p[:5], int(kind), *p[5:]))

    def tape_policy_grad(self, kind, g_params):
        """pic_tape_policy_grad into the address g_params in `kind` memory."""
        self._chk(self.lib.pic_tape_policy_grad(self._h, int(kind), _ptr(g_params)))

    # -- forward mode through the policy's steps -----------------------------------------------------------------
    def policy_jvp(self, spec, obs, pre, K, d_params, d_obs, d_pre, kind, d_pre_out, d_actions_out):
        """pic_policy_jvp on addresses (0 or None = NULL) in `kind` memory; spec as for policy_eval."""
        self._chk(self.lib.pic_policy_jvp(self._h, C.byref(spec), *_ptrs(obs, pre), int(K), *_ptrs(d_params, d_obs, d_pre), int(kind),
                                          *_ptrs(d_pre_out, d_actions_out)))

    def tape_tangent_policy(self, K, d_params, d_pre, d_actions, d_x0, d_v0, kind, d_hist, d_obs, d_pre_out, d_actions_out, d_x, d_v,
                            d_E_mesh):
        """pic_tape_tangent_policy on addresses (0 or None = NULL) in `kind` memory."""
        p = _ptrs(d_params, d_pre, d_actions, d_x0, d_v0, d_hist, d_obs, d_pre_out, d_actions_out, d_x, d_v, d_E_mesh)
        self._chk(self.lib.pic_tape_tangent_policy(self._h, int(K), *p[:5], int(kind), *p[5:]))

    def step_observe(self, E_ext=None, actions=None, nsteps=1, particles=True, out=None):
        """One Gym-style iteration in one call with one synchronisation (pic_step_observe): nsteps steps under E_ext
        [num_envs][Ng] or actions [num_envs][2*max_mode] (or neither), then -> (x, v, KE, PE, PE_reward) of the new state
        (x, v None with particles=False).  out: (x, v) C-contiguous arrays of num_envs * N elements of the particle dtype each
        to receive the particles (e.g. the two halves of one observation buffer) instead of fresh ones."""
        if E_ext is not None:
            E_ext = np.ascontiguousarray(np.asarray(E_ext, dtype=np.float64).reshape(self.num_envs, self.Ng))
        if actions is not None:
            actions = np.ascontiguousarray(np.asarray(actions, dtype=np.float64).reshape(self.num_envs, 2 * self.max_mode))
        if out is not None:
            x, v = out
            for a in (x, v):
                if a.dtype != self.dtype or a.size != self.num_envs * self.N or not a.flags.c_contiguous:
                    raise ValueError("out: two C-contiguous arrays of num_envs * N elements of the particle dtype")
        else:
            x = np.empty((self.num_envs, self.N), dtype=self.dtype) if particles else None
            v = np.empty_like(x) if particles else None
        en = np.empty((3, self.num_envs))
        self._chk(self.lib.pic_step_observe(self._h, _ptr(E_ext), _ptr(actions), int(nsteps), _ptr(x), _ptr(v),
                                            _ptr(en[0]), _ptr(en[1]), _ptr(en[2])))
        return x, v, en[0], en[1], en[2]

    def set_stream(self, hip_stream):
        """hip_stream: integer hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; 0 = the default stream)."""
        self._chk(self.lib.pic_set_stream(self._h, C.c_void_p(int(hip_stream)) if hip_stream else None))

    def own_stream(self):
        self._chk(self.lib.pic_own_stream(self._h))

    def modes_device(self, max_mode, re_ptr, im_ptr):
        self._chk(self.lib.pic_get_modes(self._h, int(max_mode), _ptr(int(re_ptr)), _ptr(int(im_ptr)), PIC_DEVICE))

    def modes(self, max_mode):
        re = np.empty((self.num_envs, int(max_mode)))
        im = np.empty_like(re)
        self._chk(self.lib.pic_get_modes(self._h, int(max_mode), _ptr(re), _ptr(im), PIC_HOST))
        return re + 1j * im

    def phase_histogram(self, nbins, vmin, vmax):
        counts = np.zeros((self.num_envs, int(nbins), int(nbins)), dtype=np.uint32)
        self._chk(self.lib.pic_phase_histogram(self._h, int(nbins), float(vmin), float(vmax), _ptr(counts)))
        return counts

    def phase_kl(self, feq, vmin, vmax):
        """KL cost of every environment's phase-space density against feq [nbins][nbins] (pic_phase_kl) -> [num_envs]."""
        f = np.ascontiguousarray(np.asarray(feq, dtype=np.float64))
        if f.ndim != 2 or f.shape[0] != f.shape[1]:
            raise ValueError("feq must be [nbins, nbins]")
        kl = np.empty(self.num_envs)
        self._chk(self.lib.pic_phase_kl(self._h, int(f.shape[0]), float(vmin), float(vmax), _ptr(f), _ptr(kl)))
        return kl

    def phase_kl_smooth(self, nx, nv, vmin, vmax, feq, feq_per_env, feq_kind, mem_kind, kl, f):
        """pic_phase_kl_smooth on addresses (int, 0 = NULL) in feq_kind / mem_kind memory."""
        spec = _phase_spec(nx, nv, vmin, vmax, feq, feq_per_env, feq_kind)
        p = _ptrs(kl, f)
        self._chk(self.lib.pic_phase_kl_smooth(self._h, C.byref(spec), int(mem_kind), p[0], p[1]))

    def phase_kl_smooth_vjp(self, nx, nv, vmin, vmax, feq, feq_per_env, feq_kind, cot_kl, mem_kind, g_x, g_v):
        """pic_phase_kl_smooth_vjp on addresses (int, 0 = NULL)."""
        spec = _phase_spec(nx, nv, vmin, vmax, feq, feq_per_env, feq_kind)
        p = _ptrs(cot_kl, g_x, g_v)
        self._chk(self.lib.pic_phase_kl_smooth_vjp(self._h, C.byref(spec), p[0], int(mem_kind), p[1], p[2]))

    def phase_kl_smooth_jvp(self, nx, nv, vmin, vmax, feq, feq_per_env, feq_kind, K, d_x, d_v, mem_kind, d_kl):
        """pic_phase_kl_smooth_jvp on addresses (int, 0 = NULL)."""
        spec = _phase_spec(nx, nv, vmin, vmax, feq, feq_per_env, feq_kind)
        p = _ptrs(d_x, d_v, d_kl)
        self._chk(self.lib.pic_phase_kl_smooth_jvp(self._h, C.byref(spec), int(K), p[0], p[1], int(mem_kind), p[2]))

    # -- rollout recorder (pic_record_*) ------------------------------------------------------------
    def record_start(self, stride=1, n_modes=0, x_bins=0, v_bins=0, phase_bins=(0, 0), vmin=-25.0, vmax=25.0, phase_dx=0.0,
                     phase_dv=0.0, feq=None, capacity=1024):
        px, pv = (int(b) for b in phase_bins)
        f = None
        if feq is not None:
            f = np.ascontiguousarray(np.asarray(feq, dtype=np.float64))
            if f.shape != (px, pv):
                raise ValueError(f"feq must be [{px}, {pv}] (the phase bins), not {list(f.shape)}")
        cfg = PicRecordConfig(int(stride), int(n_modes), int(x_bins), int(v_bins), px, pv, float(vmin), float(vmax),
                              float(phase_dx), float(phase_dv), None if f is None else f.ctypes.data, int(capacity))
        self._chk(self.lib.pic_record_start(self._h, C.byref(cfg)))
        self.record_config = {"stride": int(stride), "n_modes": int(n_modes), "x_bins": int(x_bins), "v_bins": int(v_bins),
                              "phase_bins": (px, pv), "vmin": float(vmin), "vmax": float(vmax), "feq": f is not None}

    def record_now(self):
        self._chk(self.lib.pic_record_now(self._h))

    def record_count(self):
        n = C.c_int64()
        self._chk(self.lib.pic_record_count(self._h, C.byref(n)))
        return n.value

    def record_read(self, first=0, count=None):
        """Records first..first+count-1 (all from `first` by default) -> dict of host arrays: step [R]; KE, PE, PE_reward,
        field_energy, entropy, kl, inside [R, E]; re, im [R, E, n_modes]; x_hist [R, E, x_bins], v_hist [R, E, v_bins]."""
        c = getattr(self, "record_config", None)
        if c is None:
            raise PicError("record_read: not recording")
        if count is None:
            count = self.record_count() - int(first)
        R, E = int(count), self.num_envs
        out = {"step": np.empty(R, dtype=np.int64), "inside": np.empty((R, E), dtype=np.int64)}
        for k in ("KE", "PE", "PE_reward", "field_energy", "entropy", "kl"):
            out[k] = np.empty((R, E))
        out["re"] = np.empty((R, E, c["n_modes"]))
        out["im"] = np.empty((R, E, c["n_modes"]))
        out["x_hist"] = np.empty((R, E, c["x_bins"]), dtype=np.uint32)
        out["v_hist"] = np.empty((R, E, c["v_bins"]), dtype=np.uint32)
        o = PicRecordOut(*(out[name].ctypes.data for name, _ in PicRecordOut._fields_))
        self._chk(self.lib.pic_record_read(self._h, int(first), R, C.byref(o)))
        return out

    def record_stop(self):
        self._chk(self.lib.pic_record_stop(self._h))
        self.record_config = None

    # -- differentiable rollouts (pic_tape_*) -------------------------------------------------------
    def tape_start(self, max_steps, checkpoint_every=0, budget_bytes=0):
        cfg = PicTapeConfig(int(max_steps), int(checkpoint_every), int(budget_bytes))
        self._chk(self.lib.pic_tape_start(self._h, C.byref(cfg)))
        self._taping, self._law_calls = True, []

    def tape_stats(self):
        o = PicTapeInfo()
        self._chk(self.lib.pic_tape_stats(self._h, C.byref(o)))
        return {name: int(getattr(o, name)) for name, _ in PicTapeInfo._fields_}

    def tape_backward(self, cot_hist=None, cot_x=None, cot_v=None, ext=True, actions=False, particles=False):
        """Host arrays in, host arrays out: dict with g_ext [T][num_envs][Ng], g_actions [T][num_envs][2M], g_x0 / g_v0
        [num_envs][N] (those asked for)."""
        T = self.tape_stats()["steps"]
        E = self.num_envs
        ins = [_host(cot_hist, (T, 3, E)), _host(cot_x, (E, self.N)), _host(cot_v, (E, self.N))]
        out = {}
        if ext:
            out["g_ext"] = np.zeros((T, E, self.Ng))
        if actions:
            out["g_actions"] = np.zeros((T, E, 2 * self.max_mode))
        if particles:
            out["g_x0"] = np.zeros((E, self.N))
            out["g_v0"] = np.zeros((E, self.N))
        self._tape_backward(PIC_HOST, *_addrs(*ins, *(out.get(k) for k in ("g_ext", "g_actions", "g_x0", "g_v0"))))
        return out

    def tape_backward_device(self, cot_hist, cot_x, cot_v, g_ext, g_actions, g_x0, g_v0):
        """Device pointers (0 = NULL) in and out; asynchronous on the handle's stream."""
        self._tape_backward(PIC_DEVICE, cot_hist, cot_x, cot_v, g_ext, g_actions, g_x0, g_v0)

    def _tape_backward(self, mem_kind, cot_hist, cot_x, cot_v, g_ext, g_actions, g_x0, g_v0):
        """pic_tape_backward on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(cot_hist, cot_x, cot_v, g_ext, g_actions, g_x0, g_v0)
        self._chk(self.lib.pic_tape_backward(self._h, p[0], p[1], p[2], int(mem_kind), p[3], p[4], p[5], p[6]))

    def tape_stop(self):
        self._chk(self.lib.pic_tape_stop(self._h))
        self._taping, self._law_calls = False, []

    def tape_law_calls(self):
        """(first step, steps) of every pic_step_feedback_gain call on the open tape, in order."""
        return list(self._law_calls)

    def tape_backward_feedback(self, cot_hist=None, cot_x=None, cot_v=None, cot_modes=None):
        """pic_tape_backward_feedback with host arrays: dict with g_ext, g_actions, modes [T][num_envs][2M], g_x0, g_v0."""
        T = self.tape_stats()["steps"]
        E, n = self.num_envs, 2 * self.max_mode
        ins = [_host(cot_hist, (T, 3, E)), _host(cot_x, (E, self.N)), _host(cot_v, (E, self.N)), _host(cot_modes, (T, E, n))]
        out = {"g_ext": np.zeros((T, E, self.Ng)), "g_actions": np.zeros((T, E, n)), "modes": np.zeros((T, E, n)),
               "g_x0": np.zeros((E, self.N)), "g_v0": np.zeros((E, self.N))}
        self._tape_backward_feedback(PIC_HOST, *_addrs(*ins, *(out[k] for k in ("g_ext", "g_actions", "g_x0", "g_v0", "modes"))))
        return out

    def tape_backward_feedback_device(self, cot_hist, cot_x, cot_v, cot_modes, g_ext, g_actions, g_x0, g_v0, modes):
        """Device pointers (0 = NULL) in and out; asynchronous on the handle's stream."""
        self._tape_backward_feedback(PIC_DEVICE, cot_hist, cot_x, cot_v, cot_modes, g_ext, g_actions, g_x0, g_v0, modes)

    def _tape_backward_feedback(self, mem_kind, cot_hist, cot_x, cot_v, cot_modes, g_ext, g_actions, g_x0, g_v0, modes):
        """pic_tape_backward_feedback on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(cot_hist, cot_x, cot_v, cot_modes, g_ext, g_actions, g_x0, g_v0, modes)
        self._chk(self.lib.pic_tape_backward_feedback(self._h, p[0], p[1], p[2], p[3], int(mem_kind), p[4], p[5], p[6], p[7], p[8]))

    def tape_walk_begin(self, obs_modes, mem_kind=PIC_HOST):
        self._chk(self.lib.pic_tape_walk_begin(self._h, int(obs_modes), int(mem_kind)))

    def tape_walk_step(self, cot_energies, cot_x, cot_v, cot_modes, mem_kind, g_ext, g_actions):
        """pic_tape_walk_step: addresses (int, 0 = NULL; device or host memory as mem_kind says) in and out; returns the step."""
        p = _ptrs(cot_energies, cot_x, cot_v, cot_modes, g_ext, g_actions)
        step = C.c_int64(-1)
        self._chk(self.lib.pic_tape_walk_step(self._h, p[0], p[1], p[2], p[3], int(mem_kind), p[4], p[5], C.byref(step)))
        return step.value

    def tape_walk_end(self, cot_x0, cot_v0, cot_modes0, mem_kind, g_x0, g_v0):
        """pic_tape_walk_end: addresses (int, 0 = NULL) in and out."""
        p = _ptrs(cot_x0, cot_v0, cot_modes0, g_x0, g_v0)
        self._chk(self.lib.pic_tape_walk_end(self._h, p[0], p[1], p[2], int(mem_kind), p[3], p[4]))

    def tape_tangent(self, K, d_ext=None, d_actions=None, d_x0=None, d_v0=None, fields=False, kl=False):
        """pic_tape_tangent with host arrays: K directions in, dict out with hist [K][T][3][num_envs], x / v [K][num_envs][N]
        and, with fields, E_mesh [K][T][num_envs][Ng]; with kl (pic_tape_tangent_kl), KL [K][T][num_envs]."""
        T = self.tape_stats()["steps"]
        E, K = self.num_envs, int(K)
        ins = [_host(d_ext, (K, T, E, self.Ng)), _host(d_actions, (K, T, E, -1)), _host(d_x0, (K, E, self.N)),
               _host(d_v0, (K, E, self.N))]
        out = {"hist": np.zeros((K, T, 3, E)), "x": np.zeros((K, E, self.N)), "v": np.zeros((K, E, self.N))}
        if fields:
            out["E_mesh"] = np.zeros((K, T, E, self.Ng))
        if kl:
            out["KL"] = np.zeros((K, T, E))
        self._tape_tangent(PIC_HOST, K, *_addrs(*ins, out["hist"], out["x"], out["v"], out.get("E_mesh")),
                           kl=out["KL"].ctypes.data if kl else None)
        return out

    def tape_tangent_device(self, K, d_ext, d_actions, d_x0, d_v0, hist, x, v, E_mesh):
        """pic_tape_tangent on device pointers (int, 0 = NULL); asynchronous on the handle's stream."""
        self._tape_tangent(PIC_DEVICE, K, d_ext, d_actions, d_x0, d_v0, hist, x, v, E_mesh)

    def _tape_tangent(self, mem_kind, K, d_ext, d_actions, d_x0, d_v0, hist, x, v, E_mesh, kl=None, moments=None):
        """pic_tape_tangent on addresses (int, 0 = NULL) in mem_kind memory; kl: None, or the address of d_kl (an address,
        0 = NULL, makes the call pic_tape_tangent_kl); moments: None, or the address of d_moments (an address makes the call
        pic_tape_tangent_moments)."""
        if moments is not None:
            return self.tape_tangent_moments(mem_kind, K, d_ext, d_actions, d_x0, d_v0, hist, x, v, E_mesh, kl or 0, moments)
        p = _ptrs(d_ext, d_actions, d_x0, d_v0, hist, x, v, E_mesh)
        if kl is None:
            self._chk(self.lib.pic_tape_tangent(self._h, int(K), p[0], p[1], p[2], p[3], int(mem_kind), p[4], p[5], p[6], p[7]))
        else:
            self._chk(self.lib.pic_tape_tangent_kl(self._h, int(K), p[0], p[1], p[2], p[3], int(mem_kind), p[4], p[5], p[6], p[7],
                                                   _ptrs(kl)[0]))

    def tape_kl_start(self, nx, nv, vmin, vmax, feq, feq_per_env, feq_kind):
        """pic_tape_kl_start: feq an address in feq_kind memory (the tape copies it)."""
        spec = _phase_spec(nx, nv, vmin, vmax, feq, feq_per_env, feq_kind)
        self._chk(self.lib.pic_tape_kl_start(self._h, C.byref(spec)))

    def tape_kl(self, mem_kind, kl):
        """pic_tape_kl into the address kl ([T][num_envs] float64 in mem_kind memory)."""
        self._chk(self.lib.pic_tape_kl(self._h, int(mem_kind), _ptr(int(kl)) if kl else None))

    def tape_kl_cot(self, cot_kl, mem_kind, first_step, nsteps):
        """pic_tape_kl_cot: cot_kl an address (int, 0 = NULL: clear the rows) in mem_kind memory."""
        self._chk(self.lib.pic_tape_kl_cot(self._h, _ptr(int(cot_kl)) if cot_kl else None, int(mem_kind), int(first_step),
                                           int(nsteps)))

    # -- fluid moments on the mesh (pic_moments*) ---------------------------------------
    def moments(self, mem_kind, m):
        """pic_moments into the address m ([num_envs][3][Ng] float64 in mem_kind memory)."""
        self._chk(self.lib.pic_moments(self._h, int(mem_kind), _ptr(int(m)) if m else None))

    def moments_vjp(self, cot_m, mem_kind, g_x, g_v):
        """pic_moments_vjp on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(cot_m, g_x, g_v)
        self._chk(self.lib.pic_moments_vjp(self._h, p[0], int(mem_kind), p[1], p[2]))

    def tape_moments_cot(self, cot_m, mem_kind, first_step, nsteps):
        """pic_tape_moments_cot: cot_m an address (int, 0 = NULL: clear the rows) in mem_kind memory; first_step -1 = the start."""
        self._chk(self.lib.pic_tape_moments_cot(self._h, _ptr(int(cot_m)) if cot_m else None, int(mem_kind), int(first_step),
                                                int(nsteps)))

    # -- pooled particle features (pic_pool*) -----------------------------------------------
    def pool(self, spec, x, v, mem_kind, out):
        """pic_pool on addresses (int, 0 = NULL) in mem_kind memory; spec: a PicPoolSpec."""
        p = _ptrs(x, v, out)
        self._chk(self.lib.pic_pool(self._h, C.byref(spec), p[0], p[1], int(mem_kind), p[2]))

    def pool_vjp(self, spec, x, v, cot, mem_kind, g_x, g_v, g_params):
        """pic_pool_vjp on addresses (int, 0 = NULL) in mem_kind memory; spec: a PicPoolSpec."""
        p = _ptrs(x, v, cot, g_x, g_v, g_params)
        self._chk(self.lib.pic_pool_vjp(self._h, C.byref(spec), p[0], p[1], p[2], int(mem_kind), p[3], p[4], p[5]))

    def pool_ln(self, spec, x, v, mem_kind, out):
        """pic_pool_ln on addresses (int, 0 = NULL) in mem_kind memory; spec: a PicPoolLnSpec."""
        p = _ptrs(x, v, out)
        self._chk(self.lib.pic_pool_ln(self._h, C.byref(spec), p[0], p[1], int(mem_kind), p[2]))

    def pool_ln_vjp(self, spec, x, v, cot, mem_kind, g_x, g_v, g_params):
        """pic_pool_ln_vjp on addresses (int, 0 = NULL) in mem_kind memory; spec: a PicPoolLnSpec."""
        p = _ptrs(x, v, cot, g_x, g_v, g_params)
        self._chk(self.lib.pic_pool_ln_vjp(self._h, C.byref(spec), p[0], p[1], p[2], int(mem_kind), p[3], p[4], p[5]))

    def pool_jvp(self, spec, x, v, K, d_x, d_v, d_params, mem_kind, d_out):
        """pic_pool_jvp on addresses (int, 0 = NULL) in mem_kind memory (d_params: in the spec's params_mem_kind memory); spec: a
        PicPoolSpec."""
        p = _ptrs(x, v, d_x, d_v, d_params, d_out)
        self._chk(self.lib.pic_pool_jvp(self._h, C.byref(spec), p[0], p[1], int(K), p[2], p[3], p[4], int(mem_kind), p[5]))

    def pool_ln_jvp(self, spec, x, v, K, d_x, d_v, d_params, mem_kind, d_out):
        """pic_pool_ln_jvp on addresses (int, 0 = NULL) in mem_kind memory; spec: a PicPoolLnSpec."""
        p = _ptrs(x, v, d_x, d_v, d_params, d_out)
        self._chk(self.lib.pic_pool_ln_jvp(self._h, C.byref(spec), p[0], p[1], int(K), p[2], p[3], p[4], int(mem_kind), p[5]))

    # -- forward mode of the moments and their trace on a tape ---------------------------
    def moments_jvp(self, K, d_x, d_v, mem_kind, d_m):
        """pic_moments_jvp on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(d_x, d_v, d_m)
        self._chk(self.lib.pic_moments_jvp(self._h, int(K), p[0], p[1], int(mem_kind), p[2]))

    def tape_moments_start(self):
        """pic_tape_moments_start: the moments of every taped step, on an open tape before its first step."""
        self._chk(self.lib.pic_tape_moments_start(self._h))

    def tape_moments(self, mem_kind, m):
        """pic_tape_moments into the address m ([T][num_envs][3][Ng] float64 in mem_kind memory)."""
        self._chk(self.lib.pic_tape_moments(self._h, int(mem_kind), _ptr(int(m)) if m else None))

    def tape_tangent_moments(self, mem_kind, K, d_ext, d_actions, d_x0, d_v0, hist, x, v, E_mesh, kl, moments):
        """pic_tape_tangent_moments on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(d_ext, d_actions, d_x0, d_v0, hist, x, v, E_mesh, kl, moments)
        self._chk(self.lib.pic_tape_tangent_moments(self._h, int(K), p[0], p[1], p[2], p[3], int(mem_kind), *p[4:]))

    # -- forward mode through closed loops (pic_tape_tangent_walk_*) ------------------------
    def tape_tangent_walk_begin(self, K, obs_modes, d_x0, d_v0, d_gain, mem_kind, d_modes0):
        """pic_tape_tangent_walk_begin on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(d_x0, d_v0, d_gain, d_modes0)
        self._chk(self.lib.pic_tape_tangent_walk_begin(self._h, int(K), int(obs_modes), p[0], p[1], p[2], int(mem_kind), p[3]))

    def tape_tangent_walk_step(self, d_ext, d_actions, mem_kind, d_energies, d_modes, d_actions_out, d_x, d_v, d_E_mesh):
        """pic_tape_tangent_walk_step on addresses (int, 0 = NULL) in mem_kind memory; returns the step."""
        p = _ptrs(d_ext, d_actions, d_energies, d_modes, d_actions_out, d_x, d_v, d_E_mesh)
        step = C.c_int64(-1)
        self._chk(self.lib.pic_tape_tangent_walk_step(self._h, p[0], p[1], int(mem_kind), *p[2:], C.byref(step)))
        return step.value

    def tape_tangent_walk_end(self, mem_kind, d_x, d_v):
        """pic_tape_tangent_walk_end on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(d_x, d_v)
        self._chk(self.lib.pic_tape_tangent_walk_end(self._h, int(mem_kind), p[0], p[1]))

    def tape_tangent_feedback(self, K, d_gain, d_x0, d_v0, d_actions, mem_kind, d_hist, d_modes, d_actions_out, d_x, d_v, d_E_mesh):
        """pic_tape_tangent_feedback on addresses (int, 0 = NULL) in mem_kind memory."""
        p = _ptrs(d_gain, d_x0, d_v0, d_actions, d_hist, d_modes, d_actions_out, d_x, d_v, d_E_mesh)
        self._chk(self.lib.pic_tape_tangent_feedback(self._h, int(K), p[0], p[1], p[2], p[3], int(mem_kind), *p[4:]))

    def stream_probe(self, repeats=10):
        g = C.c_double()
        self._chk(self.lib.pic_stream_probe(self._h, int(repeats), C.byref(g)))
        return g.value

    def bad_count(self):
        c = C.c_int64()
        self._chk(self.lib.pic_bad_count(self._h, C.byref(c)))
        return c.value
