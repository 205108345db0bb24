"""The Python differentiation layer (env/tape.py, env/_arrays.py) pinned without a library and without a GPU:
`_abi.Handle` is replaced by a recording fake, a BatchedPIC is constructed normally, and every method of the layer is called in
host memory.  The fake records every call (name, scalar arguments, mem kind, which addresses are null, a checksum of what it
reads at the input addresses) and writes a distinct pattern into every output, so that a case pins the order of the calls, what
reaches the library and which output buffer becomes which key of the result (the hist[:, :, 0/1/2] split and the stripped K
axis included).

EXPECTED, at the end of this file, was recorded by running `_run` of this very file over CASES against commit 3fa1a6a ("Pure step
schedule in host_schedule.h, pinned on the CPU"), the parent of the change that moved the layer out of env/batched.py, in a
separate worktree.  What the layer hands to the library is behaviour: the table is never re-recorded from
the code under test (the convention of ACCOUNTING in tests/test_gpu_adjoint.py).  The device-memory half of the layer, and
_check_replay's refusal, are covered by the GPU suite."""
import ctypes as C
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import ocplasma_amd  # noqa: F401
from ocplasma_amd import _abi
from ocplasma_amd._abi import PicError
from ocplasma_amd.control.policy import MLPPolicy, param_count
from ocplasma_amd.env import _arrays
from ocplasma_amd.env.batched import BatchedPIC

E, N, NG, M, MO, T = 2, 5, 4, 1, 2, 3
WIDTHS = (2 * MO, 3, 2 * M)
P = param_count(WIDTHS)

# Handle method -> its arguments in order: a bare name is a scalar (recorded; it also becomes a dimension of that name), "@" the
# pic_policy struct, "<name:shape" an address the call reads, ">name:shape" an address it writes.  Dimensions: E, N, Ng, n = 2M,
# T the taped steps, m = 2 M_o of a walk, nO / P / PP (= E P with per_env) of the policy, F = E for a per-environment feq.
SPEC = {
    "set_actuator": "cos sin",
    "tape_start": "max_steps every budget",
    "tape_stop": "",
    "tape_moments_start": "",
    "tape_kl_start": "nx nv vmin vmax <feq:F,nx,nv per kind",
    "tape_kl": "kind >kl:T,E",
    "tape_moments": "kind >m:T,E,3,Ng",
    "tape_kl_cot": "<cot:S,E kind first S",
    "tape_moments_cot": "<cot:S,E,3,Ng kind first S",
    "_tape_backward": "kind <hist:T,3,E <cx:E,N <cv:E,N >ext:T,E,Ng >act:T,E,n >x0:E,N >v0:E,N",
    "_tape_backward_feedback": "kind <hist:T,3,E <cx:E,N <cv:E,N <cm:T,E,n >ext:T,E,Ng >act:T,E,n >x0:E,N >v0:E,N >modes:T,E,n",
    "tape_backward_policy": "kind <hist:T,3,E <cx:E,N <cv:E,N <ca:T,E,n <co:T,E,nO >gp:PP >gu:T,E,n >go:T,E,nO >ga:T,E,n >x0:E,N "
                            ">v0:E,N",
    "tape_policy_grad": "kind >gp:PP",
    "tape_tangent_feedback": "K <dg:K,E,n,n <x0:K,E,N <v0:K,E,N <da:K,T,E,n kind >hist:K,T,3,E >dm:K,T,E,n >dao:K,T,E,n >x:K,E,N "
                             ">v:K,E,N >em:K,T,E,Ng",
    "tape_tangent_policy": "K <dp:K,PP <du:K,T,E,n <da:K,T,E,n <x0:K,E,N <v0:K,E,N kind >hist:K,T,3,E >do:K,T,E,nO >duo:K,T,E,n "
                           ">dao:K,T,E,n >x:K,E,N >v:K,E,N >em:K,T,E,Ng",
    "tape_walk_begin": "Mo",
    "tape_walk_step": "<ce:3,E <cx:E,N <cv:E,N <cm:E,m kind >gext:E,Ng >gact:E,n",
    "tape_walk_end": "<cx:E,N <cv:E,N <cm:E,m kind >x0:E,N >v0:E,N",
    "tape_tangent_walk_begin": "K Mo <x0:K,E,N <v0:K,E,N <dg:K,E,n,n kind >m0:K,E,m",
    "tape_tangent_walk_step": "<dext:K,E,Ng <da:K,E,n kind >en:K,3,E >mo:K,E,m >ao:K,E,n >x:K,E,N >v:K,E,N >em:K,E,Ng",
    "tape_tangent_walk_end": "kind >x:K,E,N >v:K,E,N",
    "policy_eval": "@ <obs:E,nO <noise:E,n <std:n kind >o:E,nO >u:E,n >a:E,n",
    "step_policy": "@ <noise:S,E,n <std:n kind S >o:S,E,nO >u:S,E,n >a:S,E,n >hist:S,3,E",
    "tape_step_policy": "@ <noise:S,E,n <std:n kind S >o:S,E,nO >u:S,E,n >a:S,E,n >hist:S,3,E",
    "policy_vjp": "@ <obs:E,nO <pre:E,n <cot:E,n kind >gp:PP >go:E,nO >gu:E,n",
    "policy_jvp": "@ <obs:E,nO <pre:E,n K <dp:K,PP <do:K,E,nO <du:K,E,n kind >duo:K,E,n >dao:K,E,n",
    "phase_kl_smooth": "nx nv vmin vmax <feq:F,nx,nv per fkind kind >kl:E >f:E,nx,nv",
    "phase_kl_smooth_vjp": "nx nv vmin vmax <feq:F,nx,nv per fkind <cot:E kind >gx:E,N >gv:E,N",
    "phase_kl_smooth_jvp": "nx nv vmin vmax <feq:F,nx,nv per fkind K <dx:K,E,N <dv:K,E,N kind >dkl:K,E",
    "moments": "kind >m:E,3,Ng",
    "moments_vjp": "<cot:E,3,Ng kind >gx:E,N >gv:E,N",
    "moments_jvp": "K <dx:K,E,N <dv:K,E,N kind >dm:K,E,3,Ng",
}
_TANGENT = "kind K <dext:K,T,E,Ng <da:K,T,E,n <x0:K,E,N <v0:K,E,N >hist:K,T,3,E >x:K,E,N >v:K,E,N >em:K,T,E,Ng"


def _view(addr, size):
    return np.ctypeslib.as_array((C.c_double * size).from_address(addr))


class FakeHandle:
    """Stands in for _abi.Handle: no library.  `log` holds one line per call."""
    made = []

    def __init__(self, N_, Ng, num_envs, *rest):
        self.dims = {"E": num_envs, "N": N_, "Ng": Ng, "n": 0, "T": 0}
        self.fixed_positions, self.log, self.law_calls, self.mismatches = False, [], [], 0
        self._walked = self._twalked = 0
        FakeHandle.made.append(self)

    def tape_stats(self):
        self.log.append("tape_stats")
        return {"steps": self.dims["T"], "replay_mismatches": self.mismatches}

    def tape_law_calls(self):
        self.log.append("tape_law_calls")
        return list(self.law_calls)

    def _tape_tangent(self, *a, kl=None, moments=None):
        spec = _TANGENT + ("" if kl is None else " >kl:K,T,E") + ("" if moments is None else " >mom:K,T,E,3,Ng")
        self._call("_tape_tangent", spec, a + (() if kl is None else (kl,)) + (() if moments is None else (moments,)))

    def tape_walk_step(self, *a):
        self._call("tape_walk_step", SPEC["tape_walk_step"], a)
        self._walked += 1
        return self.dims["T"] - self._walked

    def tape_tangent_walk_step(self, *a):
        self._call("tape_tangent_walk_step", SPEC["tape_tangent_walk_step"], a)
        self._twalked += 1
        return self._twalked - 1

    def __getattr__(self, name):
        if name not in SPEC:
            raise AttributeError(name)
        return lambda *a: self._call(name, SPEC[name], a)

    def _call(self, name, spec, args):
        tokens = spec.split()
        assert len(args) <= len(tokens), (name, len(args))
        args = tuple(args) + (None,) * (len(tokens) - len(args))
        d = self.dims
        for tok, a in zip(tokens, args):                       # the scalars first: they size the arrays
            if tok == "@":
                d["nO"], d["P"] = 2 * a.obs_modes, param_count(list(a.width)[:a.n_layers + 1])
                d["PP"] = d["P"] * (d["E"] if a.per_env else 1)
            elif tok[0] not in "<>":
                d[tok] = a
        d["m"], d["F"] = 2 * d.get("Mo", 0), d["E"] if d.get("per") else 1
        scalars, pat, crc, pos = [], "", 0, 0
        for tok, a in zip(tokens, args):
            if tok == "@":
                params = _view(a.params, d["PP"])
                scale = "-" if not a.obs_scale else "%08x" % zlib.crc32(_view(a.obs_scale, d["nO"]).tobytes())
                scalars.append("policy(%d,%d,%s,%d,%d,%d,%r,%08x,%s)" % (
                    a.obs_modes, a.n_layers, list(a.width), a.activation, a.squash, a.per_env, a.action_scale,
                    zlib.crc32(params.tobytes()), scale))
                continue
            if tok[0] not in "<>":
                scalars.append(f"{tok}={a!r}")
                continue
            shape = tuple(d[s] if s in d else int(s) for s in tok.split(":")[1].split(","))
            size = int(np.prod(shape))
            addr = a.ctypes.data if hasattr(a, "ctypes") else int(a or 0)
            if tok[0] == ">" and "|" not in pat:
                pat += "|"
            pat += "e" if size == 0 else "1" if addr else "0"
            if size and addr and tok[0] == "<":
                crc = zlib.crc32(_view(addr, size).tobytes(), crc)
            if tok[0] == ">":
                pos += 1
                if size and addr:
                    _view(addr, size)[:] = 1000.0 * pos + np.arange(size)
        self.log.append(" ".join([name] + scalars + [pat, "%08x" % crc]))


# -- inputs: exact in float64, distinct per name -----------------------------------------------------------------------------
def arr(name, shape, K=None):
    shape = ((K,) if K else ()) + tuple(shape)
    size = int(np.prod(shape))
    c = (zlib.crc32(name.encode()) % 61 + 1) / 8.0
    return ((np.arange(size) % 11 + 1) * c - 3.0).reshape(shape)


def policy(per_env=False, **kw):
    params = arr("params", (E, P) if per_env else (P,)) / 16.0
    return MLPPolicy(list(WIDTHS), "tanh", params, MO, per_env=per_env, **kw)


FEQ = arr("feq", (3, 2)) ** 2 + 1.0


def make(actuator=True, kl=False, moments=False, pol=None, steps=T, law=(), tape=True):
    """A BatchedPIC on the fake handle with an open tape of `steps` steps (taped through tape_step_policy with `pol`)."""
    env = BatchedPIC(E, N, NG)
    h = env._h
    if actuator:
        env.set_actuator(SimpleNamespace(basis_cos=None, basis_sin=None, max_mode=M))
        h.dims["n"] = 2 * M
    if tape:
        env.start_tape(8, kl=dict(feq=FEQ, vmin=-5.0) if kl else None, moments=moments)
        if pol is not None:
            env.tape_step_policy(pol, steps, history=False)
        h.dims["T"], h.law_calls = steps, list(law)
    return env


def pick(shapes, sel, K=None, **extra):
    return dict({k: arr(k, shapes[k], K) for k in sel}, **extra)


def matrix(names):
    """(label, K, present): nothing given; then each input alone and all of them, without a K axis, with K = 1 and K = 2."""
    yield "none", None, ()
    for K in (None, 1, 2):
        for sel in [(k,) for k in names] + [tuple(names)]:
            yield f"K{K}." + ("all" if len(sel) > 1 else sel[0]), K, sel


def flag_sets(*flags):
    yield {}
    for f in flags:
        yield {f: True}
    if len(flags) > 1:
        yield {f: True for f in flags}


def fl(kw):
    return "+".join(sorted(kw)) or "plain"


def _cases():
    c = {}
    n, nO = 2 * M, 2 * MO
    part = {"d_x": (E, N), "d_v": (E, N)}

    # -- tangent -----------------------------------------------------------------------------------------------------------
    def sh_tan(t):
        return {"d_ext": (t, E, NG), "d_actions": (t, E, n), "d_x0": (E, N), "d_v0": (E, N)}
    for lab, K, sel in matrix(sh_tan(T)):
        c[f"tangent.{lab}"] = lambda K=K, sel=sel: make().tangent(**pick(sh_tan(T), sel, K))
    for kw in flag_sets("fields", "kl", "moments"):
        c[f"tangent.flags.{fl(kw)}"] = lambda kw=kw: make(kl=True).tangent(**pick(sh_tan(T), sh_tan(T), 2, **kw))
        c[f"tangent.flags.noinput.{fl(kw)}"] = lambda kw=kw: make(kl=True).tangent(**kw)
    c["tangent.T0"] = lambda: make(kl=True, steps=0).tangent(**pick(sh_tan(0), sh_tan(0), 2, fields=True, kl=True, moments=True))
    c["tangent.T0.none"] = lambda: make(steps=0).tangent()
    c["tangent.no_actuator"] = lambda: make(actuator=False).tangent(d_x0=arr("d_x0", (E, N)), fields=True)
    c["tangent.err.kl"] = lambda: make().tangent(kl=True)
    c["tangent.err.disagree"] = lambda: make().tangent(d_x0=arr("d_x0", (E, N), 2), d_v0=arr("d_v0", (E, N), 3))
    c["tangent.err.shape"] = lambda: make().tangent(d_ext=arr("d_ext", (T, E, NG + 1)))
    c["tangent.err.mixed"] = lambda: make().tangent(d_x0=arr("d_x0", (E, N), 2), d_v0=arr("d_v0", (E, N)))

    # -- tangent_feedback --------------------------------------------------------------------------------------------------
    def sh_fb(t):
        return {"d_gain": (E, n, n), "d_x0": (E, N), "d_v0": (E, N), "d_actions": (t, E, n)}
    for lab, K, sel in matrix(sh_fb(T)):
        c[f"tangent_feedback.{lab}"] = lambda K=K, sel=sel: make(law=[(0, T)]).tangent_feedback(**pick(sh_fb(T), sel, K))
    c["tangent_feedback.fields"] = lambda: make().tangent_feedback(**pick(sh_fb(T), sh_fb(T), 2, fields=True))
    c["tangent_feedback.fields.none"] = lambda: make().tangent_feedback(fields=True)
    c["tangent_feedback.T0"] = lambda: make(steps=0).tangent_feedback(**pick(sh_fb(0), sh_fb(0), 2, fields=True))
    c["tangent_feedback.no_actuator"] = lambda: make(actuator=False).tangent_feedback(d_x0=arr("d_x0", (E, N), 1), fields=True)
    c["tangent_feedback.err.disagree"] = lambda: make().tangent_feedback(d_gain=arr("g", (E, n, n), 2), d_x0=arr("x", (E, N), 1))
    c["tangent_feedback.err.shape"] = lambda: make().tangent_feedback(d_gain=arr("g", (E, n, n + 1)))

    # -- backward ----------------------------------------------------------------------------------------------------------
    def sh_bw(t):
        return {"d_KE": (t, E), "d_PE": (t, E), "d_PE_reward": (t, E), "d_x": (E, N), "d_v": (E, N), "d_modes": (t, E, n),
                "d_KL": (t, E), "d_moments": (t, E, 3, NG)}
    plain = ("d_KE", "d_PE", "d_PE_reward", "d_x", "d_v")
    for sel in [()] + [(k,) for k in plain] + [plain]:
        lab = "none" if not sel else "all" if len(sel) > 1 else sel[0]
        c[f"backward.{lab}"] = lambda sel=sel: make().backward(**pick(sh_bw(T), sel))
        c[f"backward.law.{lab}"] = lambda sel=sel: make(law=[(0, T)]).backward(**pick(sh_bw(T), sel))
    c["backward.law.d_modes"] = lambda: make(law=[(0, T)]).backward(**pick(sh_bw(T), plain + ("d_modes",)))
    c["backward.law.d_modes.alone"] = lambda: make(law=[(1, 2)]).backward(**pick(sh_bw(T), ("d_modes",)))
    c["backward.law.two_calls"] = lambda: make(law=[(0, 1), (1, 2)]).backward(**pick(sh_bw(T), plain + ("d_modes",)))
    for kl in (False, True):
        for mom in (False, True):
            for sel in ((), ("d_KL",), ("d_moments",), ("d_KL", "d_moments"), plain + ("d_KL", "d_moments")):
                if "d_KL" in sel and not kl:
                    continue
                lab = f"backward.tape_kl{int(kl)}_mom{int(mom)}." + ("none" if not sel else "all" if len(sel) > 2 else "+".join(sel))
                c[lab] = lambda kl=kl, mom=mom, sel=sel: make(kl=kl, moments=mom).backward(**pick(sh_bw(T), sel))
    c["backward.law.kl.moments"] = lambda: make(kl=True, moments=True, law=[(0, T)]).backward(**pick(sh_bw(T), sh_bw(T)))

    def twice():
        env = make(kl=True)
        return [env.backward(**pick(sh_bw(T), ("d_moments", "d_KL"))), env.backward(d_x=arr("d_x", (E, N)))]
    c["backward.moments_then_cleared"] = twice
    c["backward.T0.none"] = lambda: make(kl=True, moments=True, steps=0).backward()
    c["backward.T0.all"] = lambda: make(kl=True, moments=True, steps=0).backward(**pick(sh_bw(0), plain + ("d_KL", "d_moments")))
    c["backward.no_actuator"] = lambda: make(actuator=False).backward(**pick(sh_bw(T), plain))
    c["backward.err.d_modes"] = lambda: make().backward(d_modes=arr("d_modes", (T, E, n)))
    c["backward.err.d_KL"] = lambda: make().backward(d_KL=arr("d_KL", (T, E)))

    # -- the policy's tape: tape_step_policy, backward_policy, tape_policy_grad, tangent_policy ------------------------------
    for per in (False, True):
        pe = "per_env" if per else "shared"
        for fn in ("step_policy", "tape_step_policy"):
            for sel in ((), ("noise",), ("std",), ("noise", "std")):
                for hist in (True, False):
                    def run(fn=fn, sel=sel, hist=hist, per=per):
                        env = make(tape=fn.startswith("tape"))
                        return getattr(env, fn)(policy(per), T, history=hist, **pick({"noise": (T, E, n), "std": (n,)}, sel))
                    c[f"{fn}.{pe}.{'+'.join(sel) or 'none'}.hist{int(hist)}"] = run
            c[f"{fn}.{pe}.T0"] = lambda fn=fn, per=per: getattr(make(), fn)(policy(per), 0, noise=np.zeros((0, E, n)))
        c[f"step_policy.{pe}.squash_scale"] = lambda per=per: make(tape=False).step_policy(
            policy(per, squash=True, action_scale=0.5, obs_scale=arr("os", (nO,))), 2)

        def sh_bp(t):
            return dict(sh_bw(t), d_actions=(t, E, n), d_obs=(t, E, nO))
        both = plain + ("d_actions", "d_obs")
        for sel in [()] + [(k,) for k in both] + [both]:
            lab = "none" if not sel else "all" if len(sel) > 1 else sel[0]
            c[f"backward_policy.{pe}.{lab}"] = lambda sel=sel, per=per: make(pol=policy(per)).backward_policy(**pick(sh_bp(T), sel))
        for kl in (False, True):
            for mom in (False, True):
                for sel in ((), ("d_KL",), ("d_moments",), both + ("d_KL", "d_moments")):
                    if "d_KL" in sel and not kl:
                        continue
                    lab = f"backward_policy.{pe}.tape_kl{int(kl)}_mom{int(mom)}." + ("none" if not sel else "all" if len(sel) > 2 else sel[0])
                    c[lab] = lambda kl=kl, mom=mom, sel=sel, per=per: make(kl=kl, moments=mom, pol=policy(per)).backward_policy(
                        **pick(sh_bp(T), sel))
        c[f"backward_policy.{pe}.T0"] = lambda per=per: make(kl=True, pol=policy(per), steps=0).backward_policy(
            **pick(sh_bp(0), both + ("d_KL", "d_moments")))
        c[f"tape_policy_grad.{pe}"] = lambda per=per: make(pol=policy(per)).tape_policy_grad()

        def sh_tp(t, per=per):
            return {"d_params": (E, P) if per else (P,), "d_std": (n,), "d_pre": (t, E, n), "d_actions": (t, E, n), "d_x0": (E, N),
                    "d_v0": (E, N)}
        noise = arr("noise", (T, E, n))
        for lab, K, sel in matrix(sh_tp(T)):
            c[f"tangent_policy.{pe}.{lab}"] = lambda K=K, sel=sel, per=per, sh=sh_tp(T): make(pol=policy(per)).tangent_policy(
                **pick(sh, sel, K, noise=noise if "d_std" in sel else None))
        c[f"tangent_policy.{pe}.fields"] = lambda per=per, sh=sh_tp(T): make(pol=policy(per)).tangent_policy(
            **pick(sh, sh, 2, noise=noise, fields=True))
        c[f"tangent_policy.{pe}.fields.none"] = lambda per=per: make(pol=policy(per)).tangent_policy(fields=True, noise=noise)
        c[f"tangent_policy.{pe}.T0"] = lambda per=per, sh=sh_tp(0): make(pol=policy(per), steps=0).tangent_policy(
            **pick(sh, sh, 2, noise=np.zeros((0, E, n)), fields=True))

        def sh_pj(per=per):
            return {"d_params": (E, P) if per else (P,), "d_obs": (E, nO), "d_pre": (E, n)}
        for lab, K, sel in matrix(sh_pj()):
            for pre in (False, True):
                c[f"policy_jvp.{pe}.pre{int(pre)}.{lab}"] = lambda K=K, sel=sel, per=per, pre=pre, sh=sh_pj(): make(tape=False).policy_jvp(
                    policy(per, squash=pre), arr("obs", (E, nO)), arr("pre", (E, n)) if pre else None, **pick(sh, sel, K))
        for pre in (False, True):
            c[f"policy_vjp.{pe}.pre{int(pre)}"] = lambda per=per, pre=pre: make(tape=False).policy_vjp(
                policy(per, squash=pre), arr("obs", (E, nO)), arr("cot", (E, n)), arr("pre", (E, n)) if pre else None)
        for sel in ((), ("obs",), ("noise",), ("std",), ("obs", "noise", "std")):
            c[f"policy_eval.{pe}.{'+'.join(sel) or 'none'}"] = lambda per=per, sel=sel: make(tape=False).policy_eval(
                policy(per), **pick({"obs": (E, nO), "noise": (E, n), "std": (n,)}, sel))
    c["policy.err.per_env_rows"] = lambda: make(tape=False).policy_eval(
        MLPPolicy(list(WIDTHS), "tanh", np.zeros((E + 1, P)), MO, per_env=True))
    c["backward_policy.err.no_policy"] = lambda: make().backward_policy()
    c["tape_policy_grad.err.no_policy"] = lambda: make().tape_policy_grad()
    c["tangent_policy.err.no_policy"] = lambda: make().tangent_policy()
    c["tangent_policy.err.std_without_noise"] = lambda: make(pol=policy()).tangent_policy(d_std=arr("d_std", (n,)))
    c["tangent_policy.err.disagree"] = lambda: make(pol=policy()).tangent_policy(d_x0=arr("x", (E, N), 2), d_v0=arr("v", (E, N), 1))
    c["tangent_policy.err.shape"] = lambda: make(pol=policy()).tangent_policy(d_params=arr("p", (P + 1,)))
    c["backward_policy.err.d_KL"] = lambda: make(pol=policy()).backward_policy(d_KL=arr("d_KL", (T, E)))
    c["policy_jvp.err.disagree"] = lambda: make(tape=False).policy_jvp(policy(), arr("obs", (E, nO)), d_obs=arr("o", (E, nO), 2),
                                                                        d_pre=arr("u", (E, n), 3))
    c["policy_jvp.err.shape"] = lambda: make(tape=False).policy_jvp(policy(), arr("obs", (E, nO)), d_obs=arr("o", (E, nO + 1)))
    c["policy_jvp.K8"] = lambda: make(tape=False).policy_jvp(policy(), arr("obs", (E, nO)), d_obs=arr("o", (E, nO), 8))
    c["policy_jvp.K9"] = lambda: make(tape=False).policy_jvp(policy(), arr("obs", (E, nO)), d_obs=arr("o", (E, nO), 9))

    # -- the tape itself -----------------------------------------------------------------------------------------------------
    c["start_tape.err.kl_key"] = lambda: make(tape=False).start_tape(4, kl=dict(feq=FEQ, bins=3))
    c["start_tape.per_env_feq"] = lambda: make(tape=False).start_tape(4, 2, 1 << 20, kl=dict(feq=arr("feq", (E, 3, 2)), vmax=7.0))
    c["start_tape.err.feq"] = lambda: make(tape=False).start_tape(4, kl=dict(feq=arr("feq", (E + 1, 3, 2))))

    def taping():
        env = make(tape=False)
        with env.taping(4, kl=dict(feq=FEQ), moments=True) as e:
            inside = (e is env, env._tape_kl, env._tape_mom_trace)
        return [inside, (env._tape_kl, env._tape_mom_trace, env._tape_policy)]
    c["taping"] = taping

    def stop():
        env = make(kl=True, moments=True, pol=policy())
        env.stop_tape()
        return (env._tape_kl, env._tape_moments, env._tape_mom_trace, env._tape_policy)
    c["stop_tape"] = stop
    c["tape_stats"] = lambda: make().tape_stats()
    for fn, kw in (("tape_kl", "kl"), ("tape_moments", "moments")):
        c[f"{fn}"] = lambda fn=fn, kw=kw: getattr(make(**{kw: True}), fn)()
        c[f"{fn}.T0"] = lambda fn=fn, kw=kw: getattr(make(steps=0, **{kw: True}), fn)()
        c[f"{fn}.err.closed"] = lambda fn=fn: getattr(make(), fn)()

    # -- smoothed density and KL, moments --------------------------------------------------------------------------------------
    c["phase_density_smooth.int"] = lambda: make(tape=False).phase_density_smooth(3)
    c["phase_density_smooth.pair"] = lambda: make(tape=False).phase_density_smooth((3, 2), -4.0, 6.0)
    c["kl_smooth.shared"] = lambda: make(tape=False).kl_smooth(FEQ)
    c["kl_smooth.per_env"] = lambda: make(tape=False).kl_smooth(arr("feq", (E, 3, 2)), -4.0, 6.0)
    c["kl_smooth.err.feq"] = lambda: make(tape=False).kl_smooth(arr("feq", (3,)))
    c["kl_smooth_grad.ones"] = lambda: make(tape=False).kl_smooth_grad(FEQ)
    c["kl_smooth_grad.d_kl"] = lambda: make(tape=False).kl_smooth_grad(arr("feq", (E, 3, 2)), arr("d_kl", (E,)), -4.0, 6.0)
    c["kl_smooth_grad.err.d_kl"] = lambda: make(tape=False).kl_smooth_grad(FEQ, arr("d_kl", (E + 1,)))
    for lab, K, sel in matrix(part):
        c[f"kl_smooth_jvp.{lab}"] = lambda K=K, sel=sel: make(tape=False).kl_smooth_jvp(FEQ, -4.0, 6.0, **pick(part, sel, K))
        c[f"moments_jvp.{lab}"] = lambda K=K, sel=sel: make(tape=False).moments_jvp(**pick(part, sel, K))
    for fn, args in (("kl_smooth_jvp", (FEQ,)), ("moments_jvp", ())):
        c[f"{fn}.err.disagree"] = lambda fn=fn, args=args: getattr(make(tape=False), fn)(
            *args, d_x=arr("d_x", (E, N), 2), d_v=arr("d_v", (E, N), 3))
        c[f"{fn}.K9"] = lambda fn=fn, args=args: getattr(make(tape=False), fn)(*args, d_x=arr("d_x", (E, N), 9))
    c["kl_smooth_jvp.per_env_feq"] = lambda: make(tape=False).kl_smooth_jvp(arr("feq", (E, 3, 2)), d_v=arr("d_v", (E, N), 2))
    c["moments"] = lambda: make(tape=False).moments()
    c["fluid"] = lambda: make(tape=False).fluid()
    c["moments_vjp"] = lambda: make(tape=False).moments_vjp(arr("g", (E, 3, NG)))
    c["moments_vjp.err.shape"] = lambda: make(tape=False).moments_vjp(arr("g", (E, 3, NG + 1)))

    # -- the reverse walk ------------------------------------------------------------------------------------------------------
    sh_ws = {"d_energies": (3, E), "d_x": (E, N), "d_v": (E, N), "d_modes": (E, 2 * MO), "d_kl": (E,), "d_moments": (E, 3, NG)}
    sh_we = {"d_x0": (E, N), "d_v0": (E, N), "d_modes0": (E, 2 * MO), "d_moments0": (E, 3, NG)}
    for sel in [()] + [(k,) for k in sh_ws] + [tuple(sh_ws)]:
        lab = "none" if not sel else "all" if len(sel) > 1 else sel[0]
        c[f"walk.step.{lab}"] = lambda sel=sel: make(kl=True).walk(MO).step(**pick(sh_ws, sel))
    for sel in [()] + [(k,) for k in sh_we] + [tuple(sh_we)]:
        lab = "none" if not sel else "all" if len(sel) > 1 else sel[0]
        c[f"walk.end.{lab}"] = lambda sel=sel: make().walk(MO).end(**pick(sh_we, sel))

    def full_walk(kl, mom, actuator=True, obs=MO, steps=T):
        env = make(kl=kl, moments=mom, actuator=actuator, steps=steps)
        if mom:                                                 # an earlier backward left rows on the tape
            env.backward(d_moments=arr("d_moments", (steps, E, 3, NG)))
        w = env.walk(obs)
        sel = [k for k in sh_ws if (kl or k != "d_kl") and (mom or k != "d_moments")]
        sh = dict(sh_ws, d_modes=(E, 2 * w.obs_modes))
        out = [w.step(**pick(sh, sel)) for _ in range(steps)]
        return out + [w.end(**pick(dict(sh_we, d_modes0=(E, 2 * w.obs_modes)), [k for k in sh_we if mom or k != "d_moments0"]))]
    for kl in (False, True):
        for mom in (False, True):
            c[f"walk.full.kl{int(kl)}_mom{int(mom)}"] = lambda kl=kl, mom=mom: full_walk(kl, mom)
    c["walk.full.no_actuator.default_obs"] = lambda: full_walk(False, False, actuator=False, obs=None)
    c["walk.full.T0"] = lambda: full_walk(True, True, steps=0)

    def past_the_start():
        w = make(kl=True, steps=1).walk(MO)
        return [w.step(d_kl=arr("d_kl", (E,))), w.step(d_kl=arr("d_kl", (E,)))]
    c["walk.step.kl.past_the_start"] = past_the_start
    c["walk.err.d_kl"] = lambda: make().walk(MO).step(d_kl=arr("d_kl", (E,)))

    def stale(first, then, use):
        env = make(pol=policy(), law=[(0, T)])
        w = first(env)
        then(env)
        return use(w)
    walkers = {"walk": lambda env: env.walk(MO), "tangent_walk": lambda env: env.tangent_walk(),
               "tangent_feedback": lambda env: env.tangent_feedback(), "tangent_policy": lambda env: env.tangent_policy()}
    for a in ("walk", "tangent_walk"):
        for b in walkers:
            for use in ("step", "end"):
                c[f"{a}.err.stale.{use}.after_{b}"] = lambda a=a, b=b, use=use: stale(walkers[a], walkers[b], lambda w: getattr(w, use)())
    c["walk.survives.backward_and_tangent"] = lambda: stale(walkers["walk"], lambda env: (env.backward(), env.tangent()),
                                                           lambda w: w.step())

    # -- the forward walk ------------------------------------------------------------------------------------------------------
    sh_tw = {"d_x0": (E, N), "d_v0": (E, N), "d_gain": (E, n, n)}
    sh_ts = {"d_actions": (E, n), "d_ext": (E, NG)}

    def twalk_desc(w):
        return [w.K, w.batched, w.obs_modes, w.d_modes0]
    for lab, K, sel in matrix(sh_tw):
        c[f"tangent_walk.begin.{lab}"] = lambda K=K, sel=sel: twalk_desc(make().tangent_walk(obs_modes=MO, **pick(sh_tw, sel, K)))
    for K in (1, 2, 8, 9):
        c[f"tangent_walk.begin.fixedK{K}"] = lambda K=K: twalk_desc(make().tangent_walk(K))
        c[f"tangent_walk.begin.fixedK{K}.inputs"] = lambda K=K: twalk_desc(make().tangent_walk(K, 0, **pick(sh_tw, sh_tw, K)))
    c["tangent_walk.begin.no_actuator"] = lambda: twalk_desc(make(actuator=False).tangent_walk(d_x0=arr("d_x0", (E, N), 2)))
    c["tangent_walk.err.fixedK_unbatched"] = lambda: make().tangent_walk(2, d_x0=arr("d_x0", (E, N)))
    c["tangent_walk.err.fixedK_disagree"] = lambda: make().tangent_walk(2, d_x0=arr("d_x0", (E, N), 3))
    c["tangent_walk.err.shape"] = lambda: make().tangent_walk(d_gain=arr("d_gain", (E, n, n + 1)))
    for K in (None, 1, 2):
        for sel in ((), ("d_actions",), ("d_ext",), ("d_actions", "d_ext")):
            for kw in flag_sets("state", "fields"):
                c[f"tangent_walk.step.K{K}.{'+'.join(sel) or 'none'}.{fl(kw)}"] = lambda K=K, sel=sel, kw=kw: make().tangent_walk(
                    K, MO).step(**pick(sh_ts, sel, K, **kw))

    def full_twalk(K, actuator=True, obs=MO, steps=T):
        env = make(actuator=actuator, steps=steps)
        w = env.tangent_walk(K, obs, d_x0=arr("d_x0", (E, N), K))
        out = [w.step(d_ext=arr("d_ext", (E, NG), K), state=bool(t % 2), fields=not t % 2) for t in range(steps)]
        return twalk_desc(w) + out + [w.end()]
    for K in (None, 1, 2):
        c[f"tangent_walk.full.K{K}"] = lambda K=K: full_twalk(K)
    c["tangent_walk.full.no_actuator.obs0"] = lambda: full_twalk(2, actuator=False, obs=0)
    c["tangent_walk.full.T0"] = lambda: full_twalk(2, steps=0)
    c["tangent_walk.step.err.unbatched_on_fixedK"] = lambda: make().tangent_walk(2).step(d_actions=arr("d_actions", (E, n)))
    c["tangent_walk.step.err.batched_on_unbatched"] = lambda: make().tangent_walk().step(d_actions=arr("d_actions", (E, n), 1))
    c["tangent_walk.step.err.wrongK"] = lambda: make().tangent_walk(2).step(d_ext=arr("d_ext", (E, NG), 3))
    c["tangent_walk.step.err.shape"] = lambda: make().tangent_walk().step(d_ext=arr("d_ext", (E, NG + 1)))
    return c


CASES = _cases()


def _crc(a):
    return "%08x" % zlib.crc32(np.ascontiguousarray(a, dtype=np.float64).tobytes())


def describe(r):
    """A result as text: keys in their order, shapes and a checksum of the values."""
    if isinstance(r, Exception):
        return f"raises {type(r).__name__}: {r}"
    if isinstance(r, dict):
        return "{" + " ".join(f"{k}:{describe(r[k])}" for k in r) + "}"
    if isinstance(r, (list, tuple)):
        return type(r).__name__ + "(" + " ".join(describe(x) for x in r) + ")"
    if isinstance(r, np.ndarray):
        return "x".join(map(str, r.shape)) + "=" + _crc(r)
    return repr(r)


def _run(name, monkeypatch):
    """-> (the fake handle's log, the result): what EXPECTED holds for the case."""
    monkeypatch.setattr(_abi, "Handle", FakeHandle)
    FakeHandle.made = []
    try:
        res = CASES[name]()
    except (ValueError, PicError) as e:
        res = e
    log = [line for h in FakeHandle.made for line in h.log]
    return tuple(log), describe(res)


def test_the_table_and_the_cases_are_the_same_set():
    assert sorted(EXPECTED) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_the_library_and_returns_as_recorded(name, monkeypatch):
    assert _run(name, monkeypatch) == EXPECTED[name]


def test_the_fake_is_sensitive(monkeypatch):
    """The table means something: the output patterns differ per position, inputs reach the checksum, nulls the pattern."""
    log, res = _run("tangent.K2.all", monkeypatch)
    assert len({part.split("=")[1] for part in res.strip("{}").split()}) == 5          # KE, PE, PE_reward, x, v all differ
    other, _ = _run("tangent.K2.d_x0", monkeypatch)
    assert log[-1].split()[-2:] != other[-1].split()[-2:] and log[-1].split()[-2].startswith("1111|")
    assert other[-1].split()[-2] == "0010|1110"
    assert [part.split(":")[0] for part in res.strip("{}").split()] == ["KE", "PE", "PE_reward", "x", "v"]


@pytest.mark.parametrize("fn,args", [("moments_jvp", ()), ("kl_smooth_jvp", (FEQ,))])
def test_jvp_shape_errors_name_the_argument(fn, args, monkeypatch):
    """The one text that changed with the shared parser: these two said "a tangent must have shape"; type and shapes are kept."""
    monkeypatch.setattr(_abi, "Handle", FakeHandle)
    for kw, K in (({"d_x": arr("d_x", (E, N + 1))}, None), ({"d_v": arr("d_v", (E + 1, N), 2)}, 2)):
        (k, a), = kw.items()
        want = ((K,) if K else ()) + (E, N)
        with pytest.raises(ValueError) as e:
            getattr(make(tape=False), fn)(*args, **kw)
        assert str(e.value) == f"{fn}: {k} must have shape {want}, not {a.shape}"


# -- the direction parser itself ----------------------------------------------------------------------------------------------
BASE = {"a": (E, N), "b": (T, E, 2)}


def test_directions_without_inputs_and_from_the_inputs():
    d = _arrays.directions
    assert d("f", BASE, {}) == (1, False)
    assert d("f", BASE, {"a": np.zeros((E, N))}) == (1, False)
    assert d("f", BASE, {"a": None, "b": None}) == (1, False)
    assert d("f", BASE, {"a": None, "b": np.zeros((2, T, E, 2))}) == (2, True)
    assert d("f", BASE, {"a": np.zeros((1, E, N))}) == (1, True)
    assert d("f", BASE, {"a": np.zeros((2, E, N)), "b": np.zeros((2, T, E, 2))}) == (2, True)


def test_directions_refuses_disagreeing_K_and_wrong_shapes():
    d = _arrays.directions
    with pytest.raises(ValueError, match=r"^f: the inputs disagree on the number of directions: \[2, 3\]$"):
        d("f", BASE, {"a": np.zeros((3, E, N)), "b": np.zeros((2, T, E, 2))})
    with pytest.raises(ValueError, match=r"^f: a must have shape \(2, 5\), not \(2, 6\)$"):
        d("f", BASE, {"a": np.zeros((E, N + 1))})
    with pytest.raises(ValueError, match=r"^f: b must have shape \(2, 3, 2, 2\), not \(3, 2, 2\)$"):
        d("f", BASE, {"a": np.zeros((2, E, N)), "b": np.zeros((T, E, 2))})
    with pytest.raises(ValueError, match=r"^f: the inputs disagree on the number of directions: \[2, 4\]$"):
        d("f", BASE, {"a": np.zeros((4, E, N))}, K=2)


def test_directions_does_not_cap_K():
    """K <= 8 is the library's rule (PIC_EINVAL): 9 passes through unchanged, given or read off the inputs."""
    d = _arrays.directions
    for K in (8, 9):
        assert d("f", BASE, {}, K=K) == (K, True)
        assert d("f", BASE, {"a": np.zeros((K, E, N))}) == (K, True)
        assert d("f", BASE, {"a": np.zeros((K, E, N))}, K=K) == (K, True)


def test_directions_of_a_walk_are_fixed():
    """TangentWalk.step: the walk's (K, batched) decide; an unbatched array on a walk with a K axis is refused, and so is an array
    with a K axis on a walk without one, whatever K it carries."""
    d = _arrays.directions
    assert d("f", BASE, {"a": np.zeros((2, E, N))}, walk=(2, True)) == (2, True)
    assert d("f", BASE, {"a": np.zeros((E, N))}, walk=(1, False)) == (1, False)
    assert d("f", BASE, {}, walk=(1, True)) == (1, True)
    with pytest.raises(ValueError, match=r"^f: a must have shape \(2, 2, 5\), not \(2, 5\)$"):
        d("f", BASE, {"a": np.zeros((E, N))}, walk=(2, True))
    with pytest.raises(ValueError, match=r"^f: a must have shape \(2, 5\), not \(1, 2, 5\)$"):
        d("f", BASE, {"a": np.zeros((1, E, N))}, walk=(1, False))
    with pytest.raises(ValueError, match=r"^f: a must have shape \(2, 2, 5\), not \(3, 2, 5\)$"):
        d("f", BASE, {"a": np.zeros((3, E, N))}, walk=(2, True))



# Recorded at 3fa1a6a (see the header): per case, (the fake handle's log, the result).  Never re-recorded from the code under test.
EXPECTED = {
    'backward.T0.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_law_calls',
        '_tape_backward kind=0 e11|ee11 4d99835d',
    ), '{ext:0x2x4=00000000 x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:0x2x2=00000000}'),
    'backward.T0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 e00|ee11 00000000',
    ), '{ext:0x2x4=00000000 x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:0x2x2=00000000}'),
    'backward.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 111|1111 238284b7',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.d_KE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 100|1111 e12f7127',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.d_PE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 100|1111 0898c864',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.d_PE_reward': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 100|1111 1c9cbf7e',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 001|1111 e054a19b',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 010|1111 8fa6c0f6',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.err.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
    ), 'raises ValueError: backward: d_KL needs a tape opened with kl=... (start_tape)'),
    'backward.err.d_modes': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
    ), 'raises ValueError: backward: d_modes needs steps of step_feedback_gain on the tape'),
    'backward.law.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 1110|11111 238284b7',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.d_KE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 1000|11111 e12f7127',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.d_PE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 1000|11111 0898c864',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.d_PE_reward': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 1000|11111 1c9cbf7e',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.d_modes': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 1111|11111 81e97c81',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.d_modes.alone': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 0001|11111 08dccce4',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=062504bf}'),
    'backward.law.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 0010|11111 e054a19b',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 0100|11111 8fa6c0f6',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.kl.moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 1111|11111 81e97c81',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 0000|11111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:2x2x2=ca0bdcf9}'),
    'backward.law.two_calls': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 1111|11111 81e97c81',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908 modes:3x2x2=82f46379 gain:list(2x2x2=40cd9678 2x2x2=062504bf)}'),
    'backward.moments_then_cleared': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=4 0 00000000',
        'tape_law_calls',
        '_tape_backward kind=0 010|1111 8fa6c0f6',
    ), 'list({ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908} {ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908})'),
    'backward.no_actuator': ((
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 111|1e11 238284b7',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033}'),
    'backward.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl0_mom0.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl0_mom0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl0_mom1.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl0_mom1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom0.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 111|1111 238284b7',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom0.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom0.d_KL+d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom0.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 111|1111 238284b7',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom1.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom1.d_KL+d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom1.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward.tape_kl1_mom1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
    ), '{ext:3x2x4=2149511a x0:2x5=d4d3ab29 v0:2x5=733d0033 actions:3x2x2=1396b908}'),
    'backward_policy.err.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
    ), 'raises ValueError: backward: d_KL needs a tape opened with kl=... (start_tape)'),
    'backward_policy.err.no_policy': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises PicError: backward_policy: the tape holds no steps of tape_step_policy'),
    'backward_policy.per_env.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=0 e0|eeee 00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_backward_policy kind=0 e11ee|1eee11 4d99835d',
    ), '{params:2x23=c8da64c8 pre:0x2x2=00000000 obs:0x2x4=00000000 actions:0x2x2=00000000 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 11111|111111 9e6defeb',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.d_KE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 10000|111111 e12f7127',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.d_PE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 10000|111111 0898c864',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.d_PE_reward': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 10000|111111 1c9cbf7e',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00010|111111 5f5e1f5d',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00001|111111 6ee10a65',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00100|111111 e054a19b',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 01000|111111 8fa6c0f6',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl0_mom0.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl0_mom0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl0_mom1.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl0_mom1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom0.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 11111|111111 9e6defeb',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom0.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom0.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 11111|111111 9e6defeb',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom1.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom1.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.per_env.tape_kl1_mom1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:2x23=c8da64c8 pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=0 e0|eeee 00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_backward_policy kind=0 e11ee|1eee11 4d99835d',
    ), '{params:23=4e9cdcec pre:0x2x2=00000000 obs:0x2x4=00000000 actions:0x2x2=00000000 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 11111|111111 9e6defeb',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.d_KE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 10000|111111 e12f7127',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.d_PE': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 10000|111111 0898c864',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.d_PE_reward': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 10000|111111 1c9cbf7e',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00010|111111 5f5e1f5d',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00001|111111 6ee10a65',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00100|111111 e054a19b',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 01000|111111 8fa6c0f6',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl0_mom0.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl0_mom0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl0_mom1.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl0_mom1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom0.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 11111|111111 9e6defeb',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom0.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom0.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 11111|111111 9e6defeb',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom1.d_KL': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 1 6cc01500',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom1.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'backward_policy.shared.tape_kl1_mom1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_backward_policy kind=0 00000|111111 00000000',
    ), '{params:23=4e9cdcec pre:3x2x2=1396b908 obs:3x2x4=bb972458 actions:3x2x2=56add1a8 x0:2x5=8969b80b v0:2x5=1c45384e}'),
    'fluid': ((
        'set_actuator cos=None sin=None  00000000',
        'moments kind=0 |1 00000000',
    ), 'tuple(2x4=046c614f 2x4=d5bbe39d 2x4=1865defe)'),
    'kl_smooth.err.feq': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: feq must be [nx, nv] or [num_envs, nx, nv], not [3]'),
    'kl_smooth.per_env': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth nx=3 nv=2 vmin=-4.0 vmax=6.0 per=1 fkind=0 kind=0 1|10 af2c47db',
    ), '2=47211a5d'),
    'kl_smooth.shared': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth nx=3 nv=2 vmin=-25.0 vmax=25.0 per=0 fkind=0 kind=0 1|10 d3e97b14',
    ), '2=47211a5d'),
    'kl_smooth_grad.d_kl': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_vjp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=1 fkind=0 kind=0 11|11 38c65d97',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'kl_smooth_grad.err.d_kl': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: d_kl must be [num_envs], not [3]'),
    'kl_smooth_grad.ones': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_vjp nx=3 nv=2 vmin=-25.0 vmax=25.0 per=0 fkind=0 kind=0 11|11 f0c9eb27',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'kl_smooth_jvp.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=1 kind=0 111|1 444a3a68',
    ), '1x2=47211a5d'),
    'kl_smooth_jvp.K1.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=1 kind=0 101|1 95fbfc20',
    ), '1x2=47211a5d'),
    'kl_smooth_jvp.K1.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=1 kind=0 110|1 fa099d4d',
    ), '1x2=47211a5d'),
    'kl_smooth_jvp.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=2 kind=0 111|1 858bc648',
    ), '2x2=871a1bdf'),
    'kl_smooth_jvp.K2.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=2 kind=0 101|1 165195af',
    ), '2x2=871a1bdf'),
    'kl_smooth_jvp.K2.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=2 kind=0 110|1 63ef35ed',
    ), '2x2=871a1bdf'),
    'kl_smooth_jvp.K9': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-25.0 vmax=25.0 per=0 fkind=0 K=9 kind=0 110|1 f8635010',
    ), '9x2=080f6076'),
    'kl_smooth_jvp.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=1 kind=0 111|1 444a3a68',
    ), '2=47211a5d'),
    'kl_smooth_jvp.KNone.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=1 kind=0 101|1 95fbfc20',
    ), '2=47211a5d'),
    'kl_smooth_jvp.KNone.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=1 kind=0 110|1 fa099d4d',
    ), '2=47211a5d'),
    'kl_smooth_jvp.err.disagree': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: kl_smooth_jvp: the inputs disagree on the number of directions: [2, 3]'),
    'kl_smooth_jvp.none': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 K=1 kind=0 100|1 d3e97b14',
    ), '2=47211a5d'),
    'kl_smooth_jvp.per_env_feq': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth_jvp nx=3 nv=2 vmin=-25.0 vmax=25.0 per=1 fkind=0 K=2 kind=0 101|1 8e487cc5',
    ), '2x2=871a1bdf'),
    'moments': ((
        'set_actuator cos=None sin=None  00000000',
        'moments kind=0 |1 00000000',
    ), '2x3x4=2149511a'),
    'moments_jvp.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=1 kind=0 11|1 4d99835d',
    ), '1x2x3x4=2149511a'),
    'moments_jvp.K1.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=1 kind=0 01|1 e054a19b',
    ), '1x2x3x4=2149511a'),
    'moments_jvp.K1.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=1 kind=0 10|1 8fa6c0f6',
    ), '1x2x3x4=2149511a'),
    'moments_jvp.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=2 kind=0 11|1 416087f3',
    ), '2x2x3x4=abbddd70'),
    'moments_jvp.K2.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=2 kind=0 01|1 1f822c9a',
    ), '2x2x3x4=abbddd70'),
    'moments_jvp.K2.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=2 kind=0 10|1 6a3c8cd8',
    ), '2x2x3x4=abbddd70'),
    'moments_jvp.K9': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=9 kind=0 10|1 528e0ae2',
    ), '9x2x3x4=59f7f270'),
    'moments_jvp.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=1 kind=0 11|1 4d99835d',
    ), '2x3x4=2149511a'),
    'moments_jvp.KNone.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=1 kind=0 01|1 e054a19b',
    ), '2x3x4=2149511a'),
    'moments_jvp.KNone.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=1 kind=0 10|1 8fa6c0f6',
    ), '2x3x4=2149511a'),
    'moments_jvp.err.disagree': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: moments_jvp: the inputs disagree on the number of directions: [2, 3]'),
    'moments_jvp.none': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_jvp K=1 kind=0 00|1 00000000',
    ), '2x3x4=2149511a'),
    'moments_vjp': ((
        'set_actuator cos=None sin=None  00000000',
        'moments_vjp kind=0 1|11 489e3b0a',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'moments_vjp.err.shape': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: g must be [num_envs, 3, N_mesh], not [2, 3, 5]'),
    'phase_density_smooth.int': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth nx=3 nv=3 vmin=-25.0 vmax=25.0 per=0 fkind=0 kind=0 0|01 00000000',
    ), '2x3x3=40a2f153'),
    'phase_density_smooth.pair': ((
        'set_actuator cos=None sin=None  00000000',
        'phase_kl_smooth nx=3 nv=2 vmin=-4.0 vmax=6.0 per=0 fkind=0 kind=0 0|01 00000000',
    ), '2x3x2=1396b908'),
    'policy.err.per_env_rows': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: a per-environment policy needs params [2, P], not [3, 23]'),
    'policy_eval.per_env.noise': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 010|111 9c01793e',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.per_env.none': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 000|111 00000000',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.per_env.obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 100|111 7e00cea9',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.per_env.obs+noise+std': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 111|111 d4a0da84',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.per_env.std': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 001|111 a6ee334b',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.shared.noise': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 010|111 9c01793e',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.shared.none': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 000|111 00000000',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.shared.obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 100|111 7e00cea9',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.shared.obs+noise+std': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 111|111 d4a0da84',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_eval.shared.std': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_eval policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 001|111 a6ee334b',
    ), 'tuple(2x4=dfe61479 2x2=8154b143 2x2=b8fe414a)'),
    'policy_jvp.K8': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=8 kind=0 10010|11 2ecefb37',
    ), 'tuple(8x2x2=42e992a0 8x2x2=c6af60f7)'),
    'policy_jvp.K9': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=9 kind=0 10010|11 63d4546e',
    ), 'tuple(9x2x2=a05daa8d 9x2x2=4c5eeec9)'),
    'policy_jvp.err.disagree': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: policy_jvp: the inputs disagree on the number of directions: [2, 3]'),
    'policy_jvp.err.shape': ((
        'set_actuator cos=None sin=None  00000000',
    ), 'raises ValueError: policy_jvp: d_obs must have shape (2, 4), not (2, 5)'),
    'policy_jvp.per_env.pre0.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10111|11 19e0f20f',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre0.K1.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10010|11 4d03515b',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre0.K1.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10100|11 a8883035',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre0.K1.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10001|11 2ca5f3db',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre0.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=2 kind=0 10111|11 7a127c47',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre0.K2.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=2 kind=0 10010|11 6322b948',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre0.K2.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=2 kind=0 10100|11 2c040115',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre0.K2.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=2 kind=0 10001|11 fcaa0c09',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre0.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10111|11 19e0f20f',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre0.KNone.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10010|11 4d03515b',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre0.KNone.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10100|11 a8883035',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre0.KNone.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10001|11 2ca5f3db',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) K=1 kind=0 10000|11 7e00cea9',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre1.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11111|11 d02c4741',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre1.K1.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11010|11 9a822b52',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre1.K1.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11100|11 94c175bb',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre1.K1.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11001|11 8f488e8c',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.per_env.pre1.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=2 kind=0 11111|11 94274752',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre1.K2.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=2 kind=0 11010|11 6895d1ce',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre1.K2.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=2 kind=0 11100|11 badc3637',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre1.K2.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=2 kind=0 11001|11 2b2b7600',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.per_env.pre1.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11111|11 d02c4741',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre1.KNone.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11010|11 9a822b52',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre1.KNone.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11100|11 94c175bb',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre1.KNone.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11001|11 8f488e8c',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.per_env.pre1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) K=1 kind=0 11000|11 6476d45d',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre0.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10111|11 c04cff5b',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre0.K1.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10010|11 4d03515b',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre0.K1.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10100|11 e56246b3',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre0.K1.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10001|11 2ca5f3db',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre0.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=2 kind=0 10111|11 153b0d51',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre0.K2.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=2 kind=0 10010|11 6322b948',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre0.K2.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=2 kind=0 10100|11 a8883035',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre0.K2.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=2 kind=0 10001|11 fcaa0c09',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre0.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10111|11 c04cff5b',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre0.KNone.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10010|11 4d03515b',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre0.KNone.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10100|11 e56246b3',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre0.KNone.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10001|11 2ca5f3db',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) K=1 kind=0 10000|11 7e00cea9',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre1.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11111|11 f3b92385',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre1.K1.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11010|11 9a822b52',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre1.K1.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11100|11 3ffd8328',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre1.K1.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11001|11 8f488e8c',
    ), 'tuple(1x2x2=871a1bdf 1x2x2=8154b143)'),
    'policy_jvp.shared.pre1.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=2 kind=0 11111|11 0ff59569',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre1.K2.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=2 kind=0 11010|11 6895d1ce',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre1.K2.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=2 kind=0 11100|11 94c175bb',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre1.K2.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=2 kind=0 11001|11 2b2b7600',
    ), 'tuple(2x2x2=dfe61479 2x2x2=2c261f79)'),
    'policy_jvp.shared.pre1.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11111|11 f3b92385',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre1.KNone.d_obs': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11010|11 9a822b52',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre1.KNone.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11100|11 3ffd8328',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre1.KNone.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11001|11 8f488e8c',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_jvp.shared.pre1.none': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_jvp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) K=1 kind=0 11000|11 6476d45d',
    ), 'tuple(2x2=871a1bdf 2x2=8154b143)'),
    'policy_vjp.per_env.pre0': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_vjp policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 101|111 f163506e',
    ), 'tuple(2x23=c8da64c8 2x4=2c261f79 2x2=b8fe414a)'),
    'policy_vjp.per_env.pre1': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_vjp policy(2,2,[4, 3, 2, 0, 0],0,1,1,1.0,f2f9eb64,-) kind=0 111|111 528e2d39',
    ), 'tuple(2x23=c8da64c8 2x4=2c261f79 2x2=b8fe414a)'),
    'policy_vjp.shared.pre0': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_vjp policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 101|111 f163506e',
    ), 'tuple(23=4e9cdcec 2x4=2c261f79 2x2=b8fe414a)'),
    'policy_vjp.shared.pre1': ((
        'set_actuator cos=None sin=None  00000000',
        'policy_vjp policy(2,2,[4, 3, 2, 0, 0],0,1,0,1.0,8b7b804b,-) kind=0 111|111 528e2d39',
    ), 'tuple(23=4e9cdcec 2x4=2c261f79 2x2=b8fe414a)'),
    'start_tape.err.feq': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=4 every=0 budget=0  00000000',
    ), 'raises ValueError: feq must be [nx, nv] or [num_envs, nx, nv], not [3, 3, 2]'),
    'start_tape.err.kl_key': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=4 every=0 budget=0  00000000',
    ), "raises ValueError: start_tape: unknown keys in kl: ['bins']"),
    'start_tape.per_env_feq': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=4 every=2 budget=1048576  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-25.0 vmax=7.0 per=1 kind=0 1 af2c47db',
    ), 'None'),
    'step_policy.per_env.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=0 e0|eeee 00000000',
    ), 'PolicyRollout(0x2x4=00000000 0x2x2=00000000 0x2x2=00000000 0x2=00000000 0x2=00000000 0x2=00000000)'),
    'step_policy.per_env.noise+std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 11|1110 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.per_env.noise+std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 11|1111 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'step_policy.per_env.noise.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 10|1110 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.per_env.noise.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 10|1111 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'step_policy.per_env.none.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.per_env.none.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1111 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'step_policy.per_env.squash_scale': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,1,1,0.5,f2f9eb64,9c01793e) kind=0 S=2 00|1111 00000000',
    ), 'PolicyRollout(2x2x4=94e1693b 2x2x2=2c261f79 2x2x2=72924be0 2x2=4e02a696 2x2=77fbcc29 2x2=8321badf)'),
    'step_policy.per_env.std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 01|1110 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.per_env.std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 01|1111 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'step_policy.shared.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=0 e0|eeee 00000000',
    ), 'PolicyRollout(0x2x4=00000000 0x2x2=00000000 0x2x2=00000000 0x2=00000000 0x2=00000000 0x2=00000000)'),
    'step_policy.shared.noise+std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 11|1110 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.shared.noise+std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 11|1111 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'step_policy.shared.noise.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 10|1110 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.shared.noise.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 10|1111 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'step_policy.shared.none.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.shared.none.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1111 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'step_policy.shared.squash_scale': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,1,0,0.5,8b7b804b,9c01793e) kind=0 S=2 00|1111 00000000',
    ), 'PolicyRollout(2x2x4=94e1693b 2x2x2=2c261f79 2x2x2=72924be0 2x2=4e02a696 2x2=77fbcc29 2x2=8321badf)'),
    'step_policy.shared.std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 01|1110 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'step_policy.shared.std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 01|1111 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'stop_tape': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stop  00000000',
    ), 'tuple(False False False None)'),
    'tangent.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 1111|1110 278790c4',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=931399c2 v:1x2x5=d4d3ab29}'),
    'tangent.K1.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0100|1110 5f5e1f5d',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=931399c2 v:1x2x5=d4d3ab29}'),
    'tangent.K1.d_ext': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 1000|1110 464d16b8',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=931399c2 v:1x2x5=d4d3ab29}'),
    'tangent.K1.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0001|1110 40fd156e',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=931399c2 v:1x2x5=d4d3ab29}'),
    'tangent.K1.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0010|1110 5c4b6727',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=931399c2 v:1x2x5=d4d3ab29}'),
    'tangent.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=2 1111|1110 b078bd37',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6}'),
    'tangent.K2.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=2 0100|1110 7e38767b',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6}'),
    'tangent.K2.d_ext': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=2 1000|1110 6cbf0896',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6}'),
    'tangent.K2.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=2 0001|1110 16b0bbb6',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6}'),
    'tangent.K2.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=2 0010|1110 644b1956',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6}'),
    'tangent.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 1111|1110 278790c4',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent.KNone.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0100|1110 5f5e1f5d',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent.KNone.d_ext': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 1000|1110 464d16b8',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent.KNone.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0001|1110 40fd156e',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent.KNone.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0010|1110 5c4b6727',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=2 ee11|e11eee f9db56b1',
    ), '{KE:2x0x2=00000000 PE:2x0x2=00000000 PE_reward:2x0x2=00000000 x:2x2x5=a5c43518 v:2x2x5=963186e6 E_mesh:2x0x2x4=00000000 KL:2x0x2=00000000 moments:2x0x2x3x4=00000000}'),
    'tangent.T0.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 ee00|e11e 00000000',
    ), '{KE:0x2=00000000 PE:0x2=00000000 PE_reward:0x2=00000000 x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent.err.disagree': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
    ), 'raises ValueError: tangent: the inputs disagree on the number of directions: [2, 3]'),
    'tangent.err.kl': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises PicError: tangent: kl=True needs a KL on the tape (start_tape(..., kl=...))'),
    'tangent.err.mixed': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
    ), 'raises ValueError: tangent: d_v0 must have shape (2, 2, 5), not (2, 5)'),
    'tangent.err.shape': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
    ), 'raises ValueError: tangent: d_ext must have shape (3, 2, 4), not (3, 2, 5)'),
    'tangent.flags.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=2 1111|1111 b078bd37',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6 E_mesh:2x3x2x4=d0c7cb94}'),
    'tangent.flags.fields+kl+moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=2 1111|111111 b078bd37',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6 E_mesh:2x3x2x4=d0c7cb94 KL:2x3x2=82f46379 moments:2x3x2x3x4=9aacc17a}'),
    'tangent.flags.kl': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=2 1111|11101 b078bd37',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6 KL:2x3x2=82f46379}'),
    'tangent.flags.moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=2 1111|11101 b078bd37',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6 moments:2x3x2x3x4=e6ab0503}'),
    'tangent.flags.noinput.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0000|1111 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29 E_mesh:3x2x4=e95ffe57}'),
    'tangent.flags.noinput.fields+kl+moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0000|111111 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29 E_mesh:3x2x4=e95ffe57 KL:3x2=93fb6321 moments:3x2x3x4=f9512d1b}'),
    'tangent.flags.noinput.kl': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0000|11101 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29 KL:3x2=93fb6321}'),
    'tangent.flags.noinput.moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0000|11101 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29 moments:3x2x3x4=0060c2e8}'),
    'tangent.flags.noinput.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0000|1110 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent.flags.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        '_tape_tangent kind=0 K=2 1111|1110 b078bd37',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=a5c43518 v:2x2x5=963186e6}'),
    'tangent.no_actuator': ((
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0e10|1111 5c4b6727',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29 E_mesh:3x2x4=e95ffe57}'),
    'tangent.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0000|1110 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=931399c2 v:2x5=d4d3ab29}'),
    'tangent_feedback.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 1111|111110 92ae74a4',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=733d0033 v:1x2x5=8969b80b modes:1x3x2x2=1396b908 actions:1x3x2x2=af057747}'),
    'tangent_feedback.K1.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0001|111110 5f5e1f5d',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=733d0033 v:1x2x5=8969b80b modes:1x3x2x2=1396b908 actions:1x3x2x2=af057747}'),
    'tangent_feedback.K1.d_gain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 1000|111110 b3ef2977',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=733d0033 v:1x2x5=8969b80b modes:1x3x2x2=1396b908 actions:1x3x2x2=af057747}'),
    'tangent_feedback.K1.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0010|111110 40fd156e',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=733d0033 v:1x2x5=8969b80b modes:1x3x2x2=1396b908 actions:1x3x2x2=af057747}'),
    'tangent_feedback.K1.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0100|111110 5c4b6727',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=733d0033 v:1x2x5=8969b80b modes:1x3x2x2=1396b908 actions:1x3x2x2=af057747}'),
    'tangent_feedback.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=2 kind=0 1111|111110 17ef042b',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=e78d7433 v:2x2x5=73563c8d modes:2x3x2x2=50d5ff23 actions:2x3x2x2=bb972458}'),
    'tangent_feedback.K2.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=2 kind=0 0001|111110 7e38767b',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=e78d7433 v:2x2x5=73563c8d modes:2x3x2x2=50d5ff23 actions:2x3x2x2=bb972458}'),
    'tangent_feedback.K2.d_gain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=2 kind=0 1000|111110 16299407',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=e78d7433 v:2x2x5=73563c8d modes:2x3x2x2=50d5ff23 actions:2x3x2x2=bb972458}'),
    'tangent_feedback.K2.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=2 kind=0 0010|111110 16b0bbb6',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=e78d7433 v:2x2x5=73563c8d modes:2x3x2x2=50d5ff23 actions:2x3x2x2=bb972458}'),
    'tangent_feedback.K2.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=2 kind=0 0100|111110 644b1956',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=e78d7433 v:2x2x5=73563c8d modes:2x3x2x2=50d5ff23 actions:2x3x2x2=bb972458}'),
    'tangent_feedback.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 1111|111110 92ae74a4',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=733d0033 v:2x5=8969b80b modes:3x2x2=1396b908 actions:3x2x2=af057747}'),
    'tangent_feedback.KNone.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0001|111110 5f5e1f5d',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=733d0033 v:2x5=8969b80b modes:3x2x2=1396b908 actions:3x2x2=af057747}'),
    'tangent_feedback.KNone.d_gain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 1000|111110 b3ef2977',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=733d0033 v:2x5=8969b80b modes:3x2x2=1396b908 actions:3x2x2=af057747}'),
    'tangent_feedback.KNone.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0010|111110 40fd156e',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=733d0033 v:2x5=8969b80b modes:3x2x2=1396b908 actions:3x2x2=af057747}'),
    'tangent_feedback.KNone.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0100|111110 5c4b6727',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=733d0033 v:2x5=8969b80b modes:3x2x2=1396b908 actions:3x2x2=af057747}'),
    'tangent_feedback.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=2 kind=0 111e|eee11e e6a6383f',
    ), '{KE:2x0x2=00000000 PE:2x0x2=00000000 PE_reward:2x0x2=00000000 x:2x2x5=e78d7433 v:2x2x5=73563c8d modes:2x0x2x2=00000000 actions:2x0x2x2=00000000 E_mesh:2x0x2x4=00000000}'),
    'tangent_feedback.err.disagree': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
    ), 'raises ValueError: tangent_feedback: the inputs disagree on the number of directions: [1, 2]'),
    'tangent_feedback.err.shape': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
    ), 'raises ValueError: tangent_feedback: d_gain must have shape (2, 2, 2), not (2, 2, 3)'),
    'tangent_feedback.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=2 kind=0 1111|111111 17ef042b',
    ), '{KE:2x3x2=f15b5a95 PE:2x3x2=6cac9ec7 PE_reward:2x3x2=e6daffd5 x:2x2x5=e78d7433 v:2x2x5=73563c8d modes:2x3x2x2=50d5ff23 actions:2x3x2x2=bb972458 E_mesh:2x3x2x4=069423e6}'),
    'tangent_feedback.fields.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0000|111111 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=733d0033 v:2x5=8969b80b modes:3x2x2=1396b908 actions:3x2x2=af057747 E_mesh:3x2x4=fc63c320}'),
    'tangent_feedback.no_actuator': ((
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 e10e|1ee111 5c4b6727',
    ), '{KE:1x3x2=badff747 PE:1x3x2=d13bd166 PE_reward:1x3x2=c38a3f5c x:1x2x5=733d0033 v:1x2x5=8969b80b E_mesh:1x3x2x4=fc63c320}'),
    'tangent_feedback.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0000|111110 00000000',
    ), '{KE:3x2=badff747 PE:3x2=d13bd166 PE_reward:3x2=c38a3f5c x:2x5=733d0033 v:2x5=8969b80b modes:3x2x2=1396b908 actions:3x2x2=af057747}'),
    'tangent_policy.err.disagree': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
    ), 'raises ValueError: tangent_policy: the inputs disagree on the number of directions: [1, 2]'),
    'tangent_policy.err.no_policy': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises PicError: tangent_policy: the tape holds no steps of tape_step_policy'),
    'tangent_policy.err.shape': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
    ), 'raises ValueError: tangent_policy: d_params must have shape (23,), not (24,)'),
    'tangent_policy.err.std_without_noise': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
    ), 'raises ValueError: tangent_policy: d_std needs noise, the eps of the rollout'),
    'tangent_policy.per_env.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 11111|1111110 f47ce53c',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.per_env.K1.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00100|1111110 5f5e1f5d',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.per_env.K1.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 10000|1111110 1f31f919',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.per_env.K1.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 2334531c',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.per_env.K1.d_std': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 b949ccc0',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.per_env.K1.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00001|1111110 40fd156e',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.per_env.K1.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00010|1111110 5c4b6727',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.per_env.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 11111|1111110 aabb9c05',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.per_env.K2.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 00100|1111110 7e38767b',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.per_env.K2.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 10000|1111110 a2987a64',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.per_env.K2.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 01000|1111110 c27b1412',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.per_env.K2.d_std': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 01000|1111110 08968693',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.per_env.K2.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 00001|1111110 16b0bbb6',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.per_env.K2.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 00010|1111110 644b1956',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.per_env.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 11111|1111110 f47ce53c',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.per_env.KNone.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00100|1111110 5f5e1f5d',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.per_env.KNone.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 10000|1111110 1f31f919',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.per_env.KNone.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 2334531c',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.per_env.KNone.d_std': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 b949ccc0',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.per_env.KNone.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00001|1111110 40fd156e',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.per_env.KNone.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00010|1111110 5c4b6727',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.per_env.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=0 e0|eeee 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 1ee11|eeee11e 84d0f0e3',
    ), '{dKE:2x0x2=00000000 dPE:2x0x2=00000000 dPE_reward:2x0x2=00000000 d_obs:2x0x2x4=00000000 d_pre:2x0x2x2=00000000 d_actions:2x0x2x2=00000000 d_x:2x2x5=73563c8d d_v:2x2x5=af161931 d_E_mesh:2x0x2x4=00000000}'),
    'tangent_policy.per_env.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 11111|1111111 aabb9c05',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931 d_E_mesh:2x3x2x4=42d6a364}'),
    'tangent_policy.per_env.fields.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111111 00000000',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e d_E_mesh:3x2x4=b3229380}'),
    'tangent_policy.per_env.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111110 00000000',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 11111|1111110 4d99b66f',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.shared.K1.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00100|1111110 5f5e1f5d',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.shared.K1.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 10000|1111110 f7d1e862',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.shared.K1.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 2334531c',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.shared.K1.d_std': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 b949ccc0',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.shared.K1.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00001|1111110 40fd156e',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.shared.K1.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00010|1111110 5c4b6727',
    ), '{dKE:1x3x2=badff747 dPE:1x3x2=d13bd166 dPE_reward:1x3x2=c38a3f5c d_obs:1x3x2x4=50d5ff23 d_pre:1x3x2x2=af057747 d_actions:1x3x2x2=56add1a8 d_x:1x2x5=8969b80b d_v:1x2x5=1c45384e}'),
    'tangent_policy.shared.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 11111|1111110 534b929a',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.shared.K2.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 00100|1111110 7e38767b',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.shared.K2.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 10000|1111110 1f31f919',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.shared.K2.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 01000|1111110 c27b1412',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.shared.K2.d_std': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 01000|1111110 08968693',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.shared.K2.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 00001|1111110 16b0bbb6',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.shared.K2.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 00010|1111110 644b1956',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931}'),
    'tangent_policy.shared.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 11111|1111110 4d99b66f',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.KNone.d_actions': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00100|1111110 5f5e1f5d',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.KNone.d_params': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 10000|1111110 f7d1e862',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.KNone.d_pre': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 2334531c',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.KNone.d_std': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 01000|1111110 b949ccc0',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.KNone.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00001|1111110 40fd156e',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.KNone.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00010|1111110 5c4b6727',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_policy.shared.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=0 e0|eeee 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 1ee11|eeee11e f05431d3',
    ), '{dKE:2x0x2=00000000 dPE:2x0x2=00000000 dPE_reward:2x0x2=00000000 d_obs:2x0x2x4=00000000 d_pre:2x0x2x2=00000000 d_actions:2x0x2x2=00000000 d_x:2x2x5=73563c8d d_v:2x2x5=af161931 d_E_mesh:2x0x2x4=00000000}'),
    'tangent_policy.shared.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=2 kind=0 11111|1111111 534b929a',
    ), '{dKE:2x3x2=f15b5a95 dPE:2x3x2=6cac9ec7 dPE_reward:2x3x2=e6daffd5 d_obs:2x3x2x4=9ed4d15e d_pre:2x3x2x2=bb972458 d_actions:2x3x2x2=e95ffe57 d_x:2x2x5=73563c8d d_v:2x2x5=af161931 d_E_mesh:2x3x2x4=42d6a364}'),
    'tangent_policy.shared.fields.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111111 00000000',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e d_E_mesh:3x2x4=b3229380}'),
    'tangent_policy.shared.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111110 00000000',
    ), '{dKE:3x2=badff747 dPE:3x2=d13bd166 dPE_reward:3x2=c38a3f5c d_obs:3x2x4=50d5ff23 d_pre:3x2x2=af057747 d_actions:3x2x2=56add1a8 d_x:2x5=8969b80b d_v:2x5=1c45384e}'),
    'tangent_walk.begin.K1.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 111|1 b5056969',
    ), 'list(1 True 2 1x2x4=dfe61479)'),
    'tangent_walk.begin.K1.d_gain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 001|1 b3ef2977',
    ), 'list(1 True 2 1x2x4=dfe61479)'),
    'tangent_walk.begin.K1.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 010|1 40fd156e',
    ), 'list(1 True 2 1x2x4=dfe61479)'),
    'tangent_walk.begin.K1.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 100|1 5c4b6727',
    ), 'list(1 True 2 1x2x4=dfe61479)'),
    'tangent_walk.begin.K2.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 111|1 79122505',
    ), 'list(2 True 2 2x2x4=94e1693b)'),
    'tangent_walk.begin.K2.d_gain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 001|1 16299407',
    ), 'list(2 True 2 2x2x4=94e1693b)'),
    'tangent_walk.begin.K2.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 010|1 16b0bbb6',
    ), 'list(2 True 2 2x2x4=94e1693b)'),
    'tangent_walk.begin.K2.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 100|1 644b1956',
    ), 'list(2 True 2 2x2x4=94e1693b)'),
    'tangent_walk.begin.KNone.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 111|1 b5056969',
    ), 'list(1 False 2 2x4=dfe61479)'),
    'tangent_walk.begin.KNone.d_gain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 001|1 b3ef2977',
    ), 'list(1 False 2 2x4=dfe61479)'),
    'tangent_walk.begin.KNone.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 010|1 40fd156e',
    ), 'list(1 False 2 2x4=dfe61479)'),
    'tangent_walk.begin.KNone.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 100|1 5c4b6727',
    ), 'list(1 False 2 2x4=dfe61479)'),
    'tangent_walk.begin.fixedK1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
    ), 'list(1 True 1 1x2x2=871a1bdf)'),
    'tangent_walk.begin.fixedK1.inputs': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=0 kind=0 111|e b5056969',
    ), 'list(1 True 0 None)'),
    'tangent_walk.begin.fixedK2': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=1 kind=0 000|1 00000000',
    ), 'list(2 True 1 2x2x2=dfe61479)'),
    'tangent_walk.begin.fixedK2.inputs': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=0 kind=0 111|e 79122505',
    ), 'list(2 True 0 None)'),
    'tangent_walk.begin.fixedK8': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=8 Mo=1 kind=0 000|1 00000000',
    ), 'list(8 True 1 8x2x2=42e992a0)'),
    'tangent_walk.begin.fixedK8.inputs': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=8 Mo=0 kind=0 111|e f191699a',
    ), 'list(8 True 0 None)'),
    'tangent_walk.begin.fixedK9': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=9 Mo=1 kind=0 000|1 00000000',
    ), 'list(9 True 1 9x2x2=a05daa8d)'),
    'tangent_walk.begin.fixedK9.inputs': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=9 Mo=0 kind=0 111|e 5e61fb19',
    ), 'list(9 True 0 None)'),
    'tangent_walk.begin.no_actuator': ((
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=1 kind=0 10e|1 644b1956',
    ), 'list(2 True 1 2x2x2=dfe61479)'),
    'tangent_walk.begin.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
    ), 'list(1 False 2 2x4=dfe61479)'),
    'tangent_walk.err.fixedK_disagree': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises ValueError: tangent_walk: the inputs disagree on the number of directions: [2, 3]'),
    'tangent_walk.err.fixedK_unbatched': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises ValueError: tangent_walk: d_x0 must have shape (2, 2, 5), not (2, 5)'),
    'tangent_walk.err.shape': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises ValueError: tangent_walk: d_gain must have shape (2, 2, 2), not (2, 2, 3)'),
    'tangent_walk.err.stale.end.after_tangent_feedback': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0000|111110 00000000',
    ), 'raises PicError: tangent_walk.end: another walk, backward or tangent has replaced this one'),
    'tangent_walk.err.stale.end.after_tangent_policy': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111110 00000000',
    ), 'raises PicError: tangent_walk.end: another walk, backward or tangent has replaced this one'),
    'tangent_walk.err.stale.end.after_tangent_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
    ), 'raises PicError: tangent_walk.end: another walk, backward or tangent has replaced this one'),
    'tangent_walk.err.stale.end.after_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_walk_begin Mo=2  00000000',
    ), 'raises PicError: tangent_walk.end: another walk, backward or tangent has replaced this one'),
    'tangent_walk.err.stale.step.after_tangent_feedback': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0000|111110 00000000',
    ), 'raises PicError: tangent_walk.step: another walk, backward or tangent has replaced this one'),
    'tangent_walk.err.stale.step.after_tangent_policy': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111110 00000000',
    ), 'raises PicError: tangent_walk.step: another walk, backward or tangent has replaced this one'),
    'tangent_walk.err.stale.step.after_tangent_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
    ), 'raises PicError: tangent_walk.step: another walk, backward or tangent has replaced this one'),
    'tangent_walk.err.stale.step.after_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
        'tape_walk_begin Mo=2  00000000',
    ), 'raises PicError: tangent_walk.step: another walk, backward or tangent has replaced this one'),
    'tangent_walk.full.K1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 100|1 5c4b6727',
        'tape_tangent_walk_step kind=0 10|111001 a7faf23d',
        'tape_tangent_walk_step kind=0 10|111110 a7faf23d',
        'tape_tangent_walk_step kind=0 10|111001 a7faf23d',
        'tape_tangent_walk_end kind=0 |11 00000000',
    ), 'list(1 True 2 1x2x4=dfe61479 {KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a E_mesh:1x2x4=72f8dfd0 t:0} {KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b t:1} {KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a E_mesh:1x2x4=72f8dfd0 t:2} tuple(1x2x5=c2d80ba8 1x2x5=931399c2))'),
    'tangent_walk.full.K2': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 100|1 644b1956',
        'tape_tangent_walk_step kind=0 10|111001 91013a5e',
        'tape_tangent_walk_step kind=0 10|111110 91013a5e',
        'tape_tangent_walk_step kind=0 10|111001 91013a5e',
        'tape_tangent_walk_end kind=0 |11 00000000',
    ), 'list(2 True 2 2x2x4=94e1693b {KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 E_mesh:2x2x4=7e0a505d t:0} {KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d t:1} {KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 E_mesh:2x2x4=7e0a505d t:2} tuple(2x2x5=a17bab7c 2x2x5=a5c43518))'),
    'tangent_walk.full.KNone': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 100|1 5c4b6727',
        'tape_tangent_walk_step kind=0 10|111001 a7faf23d',
        'tape_tangent_walk_step kind=0 10|111110 a7faf23d',
        'tape_tangent_walk_step kind=0 10|111001 a7faf23d',
        'tape_tangent_walk_end kind=0 |11 00000000',
    ), 'list(1 False 2 2x4=dfe61479 {KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a E_mesh:2x4=72f8dfd0 t:0} {KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b t:1} {KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a E_mesh:2x4=72f8dfd0 t:2} tuple(2x5=c2d80ba8 2x5=931399c2))'),
    'tangent_walk.full.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 100|1 644b1956',
        'tape_tangent_walk_end kind=0 |11 00000000',
    ), 'list(2 True 2 2x2x4=94e1693b tuple(2x2x5=a17bab7c 2x2x5=a5c43518))'),
    'tangent_walk.full.no_actuator.obs0': ((
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=0 kind=0 10e|e 644b1956',
        'tape_tangent_walk_step kind=0 1e|1ee001 91013a5e',
        'tape_tangent_walk_step kind=0 1e|1ee110 91013a5e',
        'tape_tangent_walk_step kind=0 1e|1ee001 91013a5e',
        'tape_tangent_walk_end kind=0 |11 00000000',
    ), 'list(2 True 0 None {KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 E_mesh:2x2x4=7e0a505d t:0} {KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 x:2x2x5=e78d7433 v:2x2x5=73563c8d t:1} {KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 E_mesh:2x2x4=7e0a505d t:2} tuple(2x2x5=a17bab7c 2x2x5=a5c43518))'),
    'tangent_walk.step.K1.d_actions+d_ext.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111001 3bf2fcec',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.d_actions+d_ext.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111111 3bf2fcec',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.d_actions+d_ext.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111000 3bf2fcec',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a t:0}'),
    'tangent_walk.step.K1.d_actions+d_ext.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111110 3bf2fcec',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b t:0}'),
    'tangent_walk.step.K1.d_actions.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111001 ab6d8302',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.d_actions.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111111 ab6d8302',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.d_actions.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111000 ab6d8302',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a t:0}'),
    'tangent_walk.step.K1.d_actions.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111110 ab6d8302',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b t:0}'),
    'tangent_walk.step.K1.d_ext.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111001 a7faf23d',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.d_ext.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111111 a7faf23d',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.d_ext.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111000 a7faf23d',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a t:0}'),
    'tangent_walk.step.K1.d_ext.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111110 a7faf23d',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b t:0}'),
    'tangent_walk.step.K1.none.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111001 00000000',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.none.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111111 00000000',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b E_mesh:1x2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.K1.none.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111000 00000000',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a t:0}'),
    'tangent_walk.step.K1.none.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111110 00000000',
    ), '{KE:1x2=47211a5d PE:1x2=f5f17de6 PE_reward:1x2=f9f0d36a modes:1x2x4=2c261f79 actions:1x2x2=b8fe414a x:1x2x5=733d0033 v:1x2x5=8969b80b t:0}'),
    'tangent_walk.step.K2.d_actions+d_ext.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111001 a9a4f741',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.d_actions+d_ext.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111111 a9a4f741',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.d_actions+d_ext.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111000 a9a4f741',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 t:0}'),
    'tangent_walk.step.K2.d_actions+d_ext.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111110 a9a4f741',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d t:0}'),
    'tangent_walk.step.K2.d_actions.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111001 b3ef2977',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.d_actions.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111111 b3ef2977',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.d_actions.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111000 b3ef2977',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 t:0}'),
    'tangent_walk.step.K2.d_actions.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111110 b3ef2977',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d t:0}'),
    'tangent_walk.step.K2.d_ext.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111001 91013a5e',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.d_ext.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111111 91013a5e',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.d_ext.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111000 91013a5e',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 t:0}'),
    'tangent_walk.step.K2.d_ext.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111110 91013a5e',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d t:0}'),
    'tangent_walk.step.K2.none.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111001 00000000',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.none.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111111 00000000',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d E_mesh:2x2x4=7e0a505d t:0}'),
    'tangent_walk.step.K2.none.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111000 00000000',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 t:0}'),
    'tangent_walk.step.K2.none.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111110 00000000',
    ), '{KE:2x2=39cbd2e8 PE:2x2=48fa560b PE_reward:2x2=2d718151 modes:2x2x4=dceda91f actions:2x2x2=72924be0 x:2x2x5=e78d7433 v:2x2x5=73563c8d t:0}'),
    'tangent_walk.step.KNone.d_actions+d_ext.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111001 3bf2fcec',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.d_actions+d_ext.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111111 3bf2fcec',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.d_actions+d_ext.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111000 3bf2fcec',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a t:0}'),
    'tangent_walk.step.KNone.d_actions+d_ext.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 11|111110 3bf2fcec',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b t:0}'),
    'tangent_walk.step.KNone.d_actions.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111001 ab6d8302',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.d_actions.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111111 ab6d8302',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.d_actions.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111000 ab6d8302',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a t:0}'),
    'tangent_walk.step.KNone.d_actions.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 01|111110 ab6d8302',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b t:0}'),
    'tangent_walk.step.KNone.d_ext.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111001 a7faf23d',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.d_ext.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111111 a7faf23d',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.d_ext.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111000 a7faf23d',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a t:0}'),
    'tangent_walk.step.KNone.d_ext.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 10|111110 a7faf23d',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b t:0}'),
    'tangent_walk.step.KNone.none.fields': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111001 00000000',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.none.fields+state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111111 00000000',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b E_mesh:2x4=72f8dfd0 t:0}'),
    'tangent_walk.step.KNone.none.plain': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111000 00000000',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a t:0}'),
    'tangent_walk.step.KNone.none.state': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=2 kind=0 000|1 00000000',
        'tape_tangent_walk_step kind=0 00|111110 00000000',
    ), '{KE:2=47211a5d PE:2=f5f17de6 PE_reward:2=f9f0d36a modes:2x4=2c261f79 actions:2x2=b8fe414a x:2x5=733d0033 v:2x5=8969b80b t:0}'),
    'tangent_walk.step.err.batched_on_unbatched': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
    ), 'raises ValueError: tangent_walk.step: d_actions must have shape (2, 2), not (1, 2, 2)'),
    'tangent_walk.step.err.shape': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
    ), 'raises ValueError: tangent_walk.step: d_ext must have shape (2, 4), not (2, 5)'),
    'tangent_walk.step.err.unbatched_on_fixedK': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=1 kind=0 000|1 00000000',
    ), 'raises ValueError: tangent_walk.step: d_actions must have shape (2, 2, 2), not (2, 2)'),
    'tangent_walk.step.err.wrongK': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_tangent_walk_begin K=2 Mo=1 kind=0 000|1 00000000',
    ), 'raises ValueError: tangent_walk.step: d_ext must have shape (2, 2, 4), not (3, 2, 4)'),
    'tape_kl': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
        'tape_kl kind=0 |1 00000000',
    ), '3x2=10b46dc9'),
    'tape_kl.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_stats',
    ), '0x2=00000000'),
    'tape_kl.err.closed': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises PicError: tape_kl: no tape with a KL is open (start_tape(..., kl=...))'),
    'tape_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_moments kind=0 |1 00000000',
    ), '3x2x3x4=d09b1a16'),
    'tape_moments.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_stats',
    ), '0x2x3x4=00000000'),
    'tape_moments.err.closed': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises PicError: tape_moments: no tape with a moments trace is open (start_tape(..., moments=True))'),
    'tape_policy_grad.err.no_policy': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
    ), 'raises PicError: tape_policy_grad: the tape holds no steps of tape_step_policy'),
    'tape_policy_grad.per_env': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
        'tape_policy_grad kind=0 |1 00000000',
    ), '2x23=c8da64c8'),
    'tape_policy_grad.shared': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_policy_grad kind=0 |1 00000000',
    ), '23=4e9cdcec'),
    'tape_stats': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_stats',
    ), '{steps:3 replay_mismatches:0}'),
    'tape_step_policy.per_env.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=0 e0|eeee 00000000',
    ), 'PolicyRollout(0x2x4=00000000 0x2x2=00000000 0x2x2=00000000 0x2=00000000 0x2=00000000 0x2=00000000)'),
    'tape_step_policy.per_env.noise+std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 11|1110 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.per_env.noise+std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 11|1111 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'tape_step_policy.per_env.noise.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 10|1110 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.per_env.noise.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 10|1111 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'tape_step_policy.per_env.none.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1110 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.per_env.none.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 00|1111 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'tape_step_policy.per_env.std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 01|1110 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.per_env.std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,1,1.0,f2f9eb64,-) kind=0 S=3 01|1111 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'tape_step_policy.shared.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=0 e0|eeee 00000000',
    ), 'PolicyRollout(0x2x4=00000000 0x2x2=00000000 0x2x2=00000000 0x2=00000000 0x2=00000000 0x2=00000000)'),
    'tape_step_policy.shared.noise+std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 11|1110 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.shared.noise+std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 11|1111 dee346e7',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'tape_step_policy.shared.noise.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 10|1110 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.shared.noise.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 10|1111 affe41dd',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'tape_step_policy.shared.none.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.shared.none.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1111 00000000',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'tape_step_policy.shared.std.hist0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 01|1110 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 None None None)'),
    'tape_step_policy.shared.std.hist1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 01|1111 a6ee334b',
    ), 'PolicyRollout(3x2x4=2149511a 3x2x2=1396b908 3x2x2=af057747 3x2=3d999650 3x2=cbd1fef6 3x2=9c14cf6f)'),
    'taping': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=4 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-25.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stop  00000000',
    ), 'list(tuple(True True True) tuple(False False None))'),
    'walk.end.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_moments_cot kind=0 first=-1 S=1 1 e5a8745a',
        'tape_walk_end kind=0 111|11 b5056969',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'walk.end.d_modes0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_walk_end kind=0 001|11 b3ef2977',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'walk.end.d_moments0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_moments_cot kind=0 first=-1 S=1 1 e5a8745a',
        'tape_walk_end kind=0 000|11 00000000',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'walk.end.d_v0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_walk_end kind=0 010|11 40fd156e',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'walk.end.d_x0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_walk_end kind=0 100|11 5c4b6727',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'walk.end.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_walk_end kind=0 000|11 00000000',
    ), 'tuple(2x5=c2d80ba8 2x5=931399c2)'),
    'walk.err.d_kl': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
    ), 'raises ValueError: walk.step: d_kl needs a tape opened with kl=... (start_tape)'),
    'walk.err.stale.end.after_tangent_feedback': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0000|111110 00000000',
    ), 'raises PicError: walk.end: another walk or backward has replaced this one'),
    'walk.err.stale.end.after_tangent_policy': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111110 00000000',
    ), 'raises PicError: walk.end: another walk or backward has replaced this one'),
    'walk.err.stale.end.after_tangent_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
    ), 'raises PicError: walk.end: another walk or backward has replaced this one'),
    'walk.err.stale.end.after_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_walk_begin Mo=2  00000000',
    ), 'raises PicError: walk.end: another walk or backward has replaced this one'),
    'walk.err.stale.step.after_tangent_feedback': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_tangent_feedback K=1 kind=0 0000|111110 00000000',
    ), 'raises PicError: walk.step: another walk or backward has replaced this one'),
    'walk.err.stale.step.after_tangent_policy': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_tangent_policy K=1 kind=0 00000|1111110 00000000',
    ), 'raises PicError: walk.step: another walk or backward has replaced this one'),
    'walk.err.stale.step.after_tangent_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_tangent_walk_begin K=1 Mo=1 kind=0 000|1 00000000',
    ), 'raises PicError: walk.step: another walk or backward has replaced this one'),
    'walk.err.stale.step.after_walk': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_walk_begin Mo=2  00000000',
    ), 'raises PicError: walk.step: another walk or backward has replaced this one'),
    'walk.full.T0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_law_calls',
        '_tape_backward kind=0 e00|ee11 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 1 e5a8745a',
        'tape_walk_end kind=0 111|11 b5056969',
    ), 'list(tuple(2x5=c2d80ba8 2x5=931399c2))'),
    'walk.full.kl0_mom0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_walk_end kind=0 111|11 b5056969',
    ), 'list(tuple(2 2x4=dfe61479 2x2=8154b143) tuple(1 2x4=dfe61479 2x2=8154b143) tuple(0 2x4=dfe61479 2x2=8154b143) tuple(2x5=c2d80ba8 2x5=931399c2))'),
    'walk.full.kl0_mom1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=4 0 00000000',
        'tape_moments_cot kind=0 first=2 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_moments_cot kind=0 first=1 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_moments_cot kind=0 first=0 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_moments_cot kind=0 first=-1 S=1 1 e5a8745a',
        'tape_walk_end kind=0 111|11 b5056969',
    ), 'list(tuple(2 2x4=dfe61479 2x2=8154b143) tuple(1 2x4=dfe61479 2x2=8154b143) tuple(0 2x4=dfe61479 2x2=8154b143) tuple(2x5=c2d80ba8 2x5=931399c2))'),
    'walk.full.kl1_mom0': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 1 74b675ff',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_kl_cot kind=0 first=1 S=1 1 74b675ff',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_kl_cot kind=0 first=0 S=1 1 74b675ff',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_walk_end kind=0 111|11 b5056969',
    ), 'list(tuple(2 2x4=dfe61479 2x2=8154b143) tuple(1 2x4=dfe61479 2x2=8154b143) tuple(0 2x4=dfe61479 2x2=8154b143) tuple(2x5=c2d80ba8 2x5=931399c2))'),
    'walk.full.kl1_mom1': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_moments_start  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=3 0 00000000',
        'tape_moments_cot kind=0 first=-1 S=1 0 00000000',
        'tape_moments_cot kind=0 first=0 S=3 1 623be06a',
        'tape_law_calls',
        '_tape_backward kind=0 000|1111 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_stats',
        'tape_moments_cot kind=0 first=-1 S=4 0 00000000',
        'tape_kl_cot kind=0 first=2 S=1 1 74b675ff',
        'tape_moments_cot kind=0 first=2 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_kl_cot kind=0 first=1 S=1 1 74b675ff',
        'tape_moments_cot kind=0 first=1 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_kl_cot kind=0 first=0 S=1 1 74b675ff',
        'tape_moments_cot kind=0 first=0 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 1111|11 83dd3077',
        'tape_moments_cot kind=0 first=-1 S=1 1 e5a8745a',
        'tape_walk_end kind=0 111|11 b5056969',
    ), 'list(tuple(2 2x4=dfe61479 2x2=8154b143) tuple(1 2x4=dfe61479 2x2=8154b143) tuple(0 2x4=dfe61479 2x2=8154b143) tuple(2x5=c2d80ba8 2x5=931399c2))'),
    'walk.full.no_actuator.default_obs': ((
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_walk_begin Mo=1  00000000',
        'tape_walk_step kind=0 1111|1e 95e9bb49',
        'tape_walk_step kind=0 1111|1e 95e9bb49',
        'tape_walk_step kind=0 1111|1e 95e9bb49',
        'tape_walk_end kind=0 111|11 cee2427f',
    ), 'list(tuple(2 2x4=dfe61479 None) tuple(1 2x4=dfe61479 None) tuple(0 2x4=dfe61479 None) tuple(2x5=c2d80ba8 2x5=931399c2))'),
    'walk.step.all': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 1 74b675ff',
        'tape_stats',
        'tape_moments_cot kind=0 first=2 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 1111|11 83dd3077',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.step.d_energies': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 0 00000000',
        'tape_walk_step kind=0 1000|11 30e12341',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.step.d_kl': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 1 74b675ff',
        'tape_walk_step kind=0 0000|11 00000000',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.step.d_modes': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 0 00000000',
        'tape_walk_step kind=0 0001|11 d04f8bd8',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.step.d_moments': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 0 00000000',
        'tape_stats',
        'tape_moments_cot kind=0 first=2 S=1 1 6de4e9c6',
        'tape_walk_step kind=0 0000|11 00000000',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.step.d_v': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 0 00000000',
        'tape_walk_step kind=0 0010|11 e054a19b',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.step.d_x': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 0 00000000',
        'tape_walk_step kind=0 0100|11 8fa6c0f6',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.step.kl.past_the_start': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=0 S=1 1 74b675ff',
        'tape_walk_step kind=0 0000|11 00000000',
        'tape_walk_step kind=0 0000|11 00000000',
    ), 'list(tuple(0 2x4=dfe61479 2x2=8154b143) tuple(-1 2x4=dfe61479 2x2=8154b143))'),
    'walk.step.none': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_kl_start nx=3 nv=2 vmin=-5.0 vmax=25.0 per=0 kind=0 1 d3e97b14',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_kl_cot kind=0 first=2 S=1 0 00000000',
        'tape_walk_step kind=0 0000|11 00000000',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
    'walk.survives.backward_and_tangent': ((
        'set_actuator cos=None sin=None  00000000',
        'tape_start max_steps=8 every=0 budget=0  00000000',
        'tape_step_policy policy(2,2,[4, 3, 2, 0, 0],0,0,0,1.0,8b7b804b,-) kind=0 S=3 00|1110 00000000',
        'tape_walk_begin Mo=2  00000000',
        'tape_stats',
        'tape_law_calls',
        '_tape_backward_feedback kind=0 0000|11111 00000000',
        'tape_stats',
        '_tape_tangent kind=0 K=1 0000|1110 00000000',
        'tape_walk_step kind=0 0000|11 00000000',
    ), 'tuple(2 2x4=dfe61479 2x2=8154b143)'),
}
