"""Cost of a closed loop under the DeepSets particle actor: wall time per step, host clock around work that ends
in a device synchronise (profiles/policy_rollout.py's method), of

  a  step_actor: the pool, the head and the steps in one call
  b  the Python loop (x, v) copies -> the actor's torch twin (PoolEncoder + torch layers) -> step_actions_torch on a stream shared
     with torch (no host wait): the route without this call
  c  step_actions_traj with precomputed actions: the steps with no actor at all
  k  pic_actor_eval on given features, back to back on the device: one launch of actor_kernel per call
  p  pic_pool_ln on the stored particles, back to back: the pool's max pass, pass and finish

under a reference-shaped actor (phi = Linear(3, 64) -> LayerNorm -> ReLU, the mean, four Linear(64, 64) -> LayerNorm -> ReLU
layers and a last Linear(64, 6) under a rescaled tanh; M = 3) at 64 x 5000 and 256 x 5000 (Ng 250) and config 2's shape
(64 x 1e6, Ng 256).  A timed window is a few calls of T steps each, back to back.  The variants alternate within every round;
per variant the median, the fastest and the slowest round are reported, in microseconds per step.  One JSON line per shape.

    python profiles/actor_rollout.py [--shape small|ref|cfg2|all] [--variants abckp] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402

SHAPES = {"small": (64, 5000, 250, 100, 10), "ref": (256, 5000, 250, 100, 10), "cfg2": (64, 1_000_000, 256, 20, 2)}   # E, N, Ng, T, calls per timed window
M, H = 3, 64


def reference_shaped_actor(rng):
    from ocplasma_amd.control.actor import ParticleActor
    norm = lambda n: (rng.uniform(0.5, 1.5, n), rng.uniform(-0.5, 0.5, n))
    layers = [(rng.normal(size=(H, H)) / np.sqrt(H), 0.1 * rng.normal(size=H), *norm(H)) for _ in range(4)]
    layers.append((rng.normal(size=(2 * M, H)) / np.sqrt(H), 0.1 * rng.normal(size=2 * M), None, None))
    g, be = norm(H)
    return ParticleActor(0.5 * rng.normal(size=(H, 3)), 0.1 * rng.normal(size=H), ParticleActor.widths_of(layers), ParticleActor.pack(layers),
                         "relu", gamma=g, beta=be, v_scale=0.1, layernorm=True, squash=True, action_scale=0.5)


def measure(E, N, Ng, T, calls, variants, rounds):
    import torch
    from ocplasma_amd.env._arrays import Mem
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.set_actuator(E_field(50.0, Ng, M))
    env.use_torch_stream()
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(0)
    host = reference_shaped_actor(rng)
    actor = host.with_params(torch.tensor(host.params, **f64))
    twin = host.to_torch(env)
    mem = Mem.of(env, force_device=True)
    spec, keep = actor.spec(mem, E)
    feats = torch.rand((E, H), **f64)
    outs = [torch.empty((E, 2 * M), **f64) for _ in range(2)]
    pooled = torch.empty((E, H), **f64)

    def run_a():
        env.step_actor(actor, T, history=False, on_device=True)

    views = env.torch_views()            # zero-copy x, v [E, N]; on the shared stream the stream orders the reads behind the steps
    state = lambda: tuple(views[k].clone(memory_format=torch.contiguous_format) for k in ("x", "v"))      # (rollout_policy's o_t)

    def run_b():
        with torch.no_grad():
            for _ in range(T):
                env.step_actions_torch(twin(state()).contiguous())

    def run_k():
        for _ in range(T):
            env._h.actor_eval(spec, feats.data_ptr(), 0, 0, 0, 0, mem.kind, 0, *(o.data_ptr() for o in outs))

    def run_p():
        for _ in range(T):
            env._h.pool_ln(spec.pool_ln.contents, 0, 0, mem.kind, pooled.data_ptr())

    acts = torch.tensor(rng.uniform(-0.5, 0.5, (T, E, 2 * M)), **f64)
    runs = dict(a=run_a, b=run_b, c=lambda: env.step_actions_traj_torch(acts), k=run_k, p=run_p)
    order = [v for v in variants if v in runs]
    times = {v: [] for v in order}
    for v in order:                      # warm-up: code objects, torch's kernels, the handle's buffers
        runs[v]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v in order:                  # interleaved: drift and neighbours hit every variant alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                runs[v]()
            torch.cuda.synchronize()
            times[v].append(1e6 * (time.perf_counter() - t0) / (T * calls))
    out = {"E": E, "N": N, "Ng": Ng, "T": T, "calls_per_window": calls, "rounds": rounds, "schedule": env._h.schedule(), "bad": env.bad_count()}
    for v in order:
        t = sorted(times[v])
        out[v] = {"median_us": round(t[len(t) // 2], 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2)}
    med = lambda v: out[v]["median_us"]
    if "a" in out and "b" in out:
        out["a_over_b"] = round(med("a") / med("b"), 3)
    if "a" in out and "c" in out:
        out["a_minus_c_us"] = round(med("a") - med("c"), 2)
    del keep
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["small", "ref", "cfg2", "all"])
    ap.add_argument("--variants", default="abckp")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    for name in (("small", "ref", "cfg2") if args.shape == "all" else (args.shape,)):
        print(json.dumps({"shape": name, **measure(*SHAPES[name], args.variants, args.rounds)}), flush=True)


if __name__ == "__main__":
    main()
