"""Forward mode through an MLP policy on the device: cost and the references' own accuracy.

Timing (default): wall time of one pass (reset, taped forward, tangent), host clock around work that ends in a device synchronise, of

  a  start_tape + tape_step_policy, then one tangent_policy with K directions in the parameters (policy_jvp_kernel in the walk)
  b  env.grad.rollout_policy_jvp under the policy's float64 torch twin: back to Python every step (the route a replaces)
  c  an open-loop tape of the same length (step_actions_traj) and one pic_tape_tangent with K directions in the actions: the floor
  k  pic_policy_jvp, back to back on the device: one launch of policy_jvp_kernel per call

under a [6, 64, 64, 6] tanh policy (M = M_o = 3) at 256 x 5000 (Ng 250, T = 100; K = 1, 4, 8) and config 2's shape (64 x 1e6,
Ng 256, T = 20; K = 1).  The variants alternate within every round; per variant the median, the fastest and the slowest round:
a, b, c in milliseconds per pass, k in microseconds per call.  One JSON line per shape and K.

--accuracy: what the bounds of tests/test_gpu_policy_jvp.py are taken from, at that test's shapes -- quantities of code that was
there before forward mode through the policy, never of tangent_policy itself:
  twin_vs_forward_mode   rollout_policy_jvp under the twin against torch forward mode of tests/hp_policy.py on the CPU
  twin_duality_gap       rollout_policy_jvp against the backward of rollout_policy under the same twin

    python profiles/policy_jvp_device.py [--shape ref|cfg2|all] [--variants abck] [--rounds 5] [--accuracy]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402

SHAPES = {"ref": (256, 5000, 250, 100, (1, 4, 8)), "cfg2": (64, 1_000_000, 256, 20, (1,))}   # E, N, Ng, T, Ks
M = 3
WIDTHS = [2 * M, 64, 64, 2 * M]
L = 50.0


def measure(E, N, Ng, T, K, variants, rounds):
    import torch
    from ocplasma_amd.control.policy import MLPPolicy, param_count
    from ocplasma_amd.env import grad
    from ocplasma_amd.env._arrays import Mem
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    env.set_actuator(E_field(L, Ng, M))
    env.use_torch_stream()
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(0)
    pol = MLPPolicy(WIDTHS, "tanh", torch.tensor(0.1 * rng.standard_normal(param_count(WIDTHS)), **f64), M,
                    obs_scale=torch.full((2 * M,), 8.0, **f64))
    net = pol.to_torch().to("cuda")
    names = [n for n, _ in net.named_parameters()]
    tparams = {n: p.detach() for n, p in net.named_parameters()}
    d_flat = torch.tensor(rng.standard_normal((K, pol.n_params)), **f64)
    d_twin = []
    for k in range(K):
        layers = pol.unpack(d_flat[k])
        d = {}
        for l, (dW, db) in enumerate(layers):
            d[f"{2 * l}.weight"], d[f"{2 * l}.bias"] = torch.tensor(dW, **f64), torch.tensor(db, **f64)
        assert sorted(d) == sorted(names)
        d_twin.append(d)
    acts0 = torch.tensor(rng.uniform(-0.5, 0.5, (T, E, 2 * M)), **f64)
    d_acts = torch.tensor(rng.standard_normal((K, T, E, 2 * M)), **f64)

    def fresh():
        env.stop_tape()
        env.reset_sampled("two-stream", seed=1)

    def run_a():
        fresh()
        env.start_tape(T)
        env.tape_step_policy(pol, T, history=False, on_device=True)
        env.tangent_policy(d_params=d_flat)

    def twin(p, o):
        return pol.torch_actions(lambda x: torch.func.functional_call(net, p, (x,)), o)

    def run_b():
        fresh()
        grad.rollout_policy_jvp(env, twin, tparams, d_twin, T, observe="modes", obs_modes=M)

    def run_c():
        fresh()
        env.start_tape(T)
        env.step_actions_traj_torch(acts0)
        env.tangent(d_actions=d_acts)

    mem = Mem.of(env, force_device=True)
    spec, keep = pol.spec(mem, E)
    obs, pre = (torch.tensor(rng.standard_normal((E, n)), **f64) for n in (2 * M, 2 * M))
    d_obs = torch.tensor(rng.standard_normal((K, E, 2 * M)), **f64)
    du, da = torch.empty((K, E, 2 * M), **f64), torch.empty((K, E, 2 * M), **f64)

    def run_k():
        for _ in range(T):
            env._h.policy_jvp(spec, obs.data_ptr(), pre.data_ptr(), K, d_flat.data_ptr(), d_obs.data_ptr(), 0, mem.kind,
                              du.data_ptr(), da.data_ptr())

    runs = {"a": run_a, "b": run_b, "c": run_c, "k": run_k}
    order = [v for v in variants if v in runs]
    times = {v: [] for v in order}
    for v in order:                      # warm-up: code objects, torch's kernels, the handle's buffers
        runs[v]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v in order:                  # interleaved: drift and neighbours hit every variant alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[v]()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            times[v].append(1e6 * dt / T if v == "k" else 1e3 * dt)
    launches = None
    if "a" in order:
        run_a()
        launches = env.tape_stats()["launches"]
    env.stop_tape()
    out = {"E": E, "N": N, "Ng": Ng, "T": T, "K": K, "rounds": rounds, "schedule": env._h.schedule(), "bad": env.bad_count(),
           "tangent_policy_launches": launches, "units": {"a": "ms", "b": "ms", "c": "ms", "k": "us per call"}}
    for v in order:
        t = sorted(times[v])
        out[v] = {"median": round(t[len(t) // 2], 3), "min": round(t[0], 3), "max": round(t[-1], 3)}
    med = lambda v: out[v]["median"]  # noqa: E731
    if "a" in out and "b" in out:
        out["a_over_b"] = round(med("a") / med("b"), 3)
    if "a" in out and "c" in out:
        out["a_minus_c_us_per_step"] = round(1e3 * (med("a") - med("c")) / T, 2)
    env.close()
    return out


def accuracy():
    """The two reference figures at the shapes of tests/test_gpu_policy_jvp.py (its own helpers build the cases)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hp_policy_jvp_routes as routes
    import test_gpu_policy_jvp as tj
    from ocplasma_amd.env import grad
    out = {}
    T, E, N, K = tj.T6, tj.E3, tj.N3, 2
    for bpe, Ng, Mo in ((-1, 33, 2), (4, 250, 5)):
        pol = tj._rollout_policy(Mo)
        eps, std = tj._noise()
        d = tj._directions(pol, K)
        twin = routes.Twin(pol, eps, std)
        X, V = tj._start(E, N)
        dx, dv = (torch.as_tensor(d[k], device="cuda") for k in ("d_x0", "d_v0"))
        for every in (1, 0):
            env = tj._make(E, N, Ng, blocks_per_env=bpe)
            got = routes.twin_route(env, twin, d["d_params"], d["d_std"], T, dx, dv, checkpoint_every=every)
            env.stop_tape()
            env.close()
            hist, acts = routes.oracle_route(X, V, twin, d["d_params"], d["d_std"], T, Ng, tj.L, 0.1, tj.M, d["d_x0"], d["d_v0"])
            errs = {"dKE": tj.rel_err(got["dKE"], hist[:, :, 0]), "dPE": tj.rel_err(got["dPE"], hist[:, :, 1]),
                    "dPE_reward": tj.rel_err(got["dPE_reward"], hist[:, :, 2]), "d_actions": tj.rel_err(got["d_actions"], acts)}
            out[f"twin_vs_forward_mode.bpe{bpe}.Ng{Ng}.every{every}"] = errs
        # the existing dual pair: the twin's backward against the twin's forward mode, directions in the parameters and std
        env = tj._make(E, N, Ng, blocks_per_env=bpe)
        p = {k: a.clone().requires_grad_(True) for k, a in twin.params("cuda").items()}
        fn = twin.fn(T, 1, "cuda")
        ke, pe, per, acts, _ = grad.rollout_policy(env, lambda o: fn(p, o), T, observe="modes", obs_modes=Mo, checkpoint_every=2)
        g = torch.Generator().manual_seed(9)
        w_hist = torch.randn((3, T, E), generator=g, dtype=torch.float64).to("cuda")
        w_act = torch.randn((T, E, 2 * tj.M), generator=g, dtype=torch.float64).to("cuda")
        ((torch.stack([ke, pe, per]) * w_hist).sum() + (acts * w_act).sum()).backward()
        env.stop_tape()
        env.reset(X, V)
        fw = routes.twin_route(env, twin, d["d_params"], d["d_std"], T, checkpoint_every=2)
        env.stop_tape()
        env.close()
        gaps = []
        for k in range(K):
            lhs = float((np.stack([fw["dKE"][k], fw["dPE"][k], fw["dPE_reward"][k]]) * w_hist.cpu().numpy()).sum()
                        + (fw["d_actions"][k] * w_act.cpu().numpy()).sum())
            dk = twin.direction(d["d_params"][k], d["d_std"][k], "cuda")
            rhs = float(sum((p[n].grad * dk[n]).sum() for n in p))
            gaps.append(abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        out[f"twin_duality_gap.bpe{bpe}.Ng{Ng}"] = gaps
    worst = max(v for k, e in out.items() if k.startswith("twin_vs") for v in e.values())
    print(json.dumps({"accuracy": out, "twin_vs_forward_mode": worst,
                      "twin_duality_gap": max(v for k, e in out.items() if k.startswith("twin_dual") for v in e)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["ref", "cfg2", "all"])
    ap.add_argument("--variants", default="abck")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    if args.accuracy:
        accuracy()
        return
    for name in (("ref", "cfg2") if args.shape == "all" else (args.shape,)):
        E, N, Ng, T, Ks = SHAPES[name]
        for K in Ks:
            print(json.dumps({"shape": name, **measure(E, N, Ng, T, K, args.variants, args.rounds)}), flush=True)


if __name__ == "__main__":
    main()
