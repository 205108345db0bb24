"""Sampling-based receding-horizon control on copies of the plant.

`MPPI` keeps a nominal action sequence.  Every `plan()` clones the plant's present state into `samples` environments
(`BatchedPIC.copy_from`: the clones continue bit for bit like the plant), rolls out `samples` perturbed sequences in one
call, and moves the nominal towards the cheap ones with softmin weights.  `act()` steps the plant under the nominal's first
action and shifts the nominal by one step.  Because a clone's rollout IS what the plant would do, sample 0 -- the nominal
itself -- predicts the plant exactly.

The arithmetic of the update (`mppi_draw`, `mppi_weights`, `mppi_update`, `mppi_shift`, `default_cost`) is plain NumPy and
needs no device.
"""
from typing import Callable, Optional

import numpy as np


def mppi_draw(nominal, samples: int, sigma: float, rng):
    """actions [horizon, samples, A] = nominal [horizon, A] + sigma * standard normal draws; sample 0 is the nominal itself."""
    nominal = np.asarray(nominal, dtype=np.float64)
    noise = rng.standard_normal((nominal.shape[0], int(samples), nominal.shape[1]))
    noise[:, 0, :] = 0.0
    return nominal[:, None, :] + float(sigma) * noise


def mppi_weights(costs, temperature: float):
    """Softmin weights of costs [samples]: exp(-(c - min c) / temperature), normalised to sum 1."""
    c = np.asarray(costs, dtype=np.float64)
    w = np.exp(-(c - c.min()) / float(temperature))
    return w / w.sum()


def mppi_update(actions, weights):
    """The weighted mean over the samples of actions [horizon, samples, A] -> the new nominal [horizon, A]."""
    return np.einsum("tka,k->ta", np.asarray(actions, dtype=np.float64), np.asarray(weights, dtype=np.float64))


def mppi_shift(nominal):
    """The nominal one step on: row t + 1 becomes row t, the new last row is zero (no control)."""
    nominal = np.asarray(nominal, dtype=np.float64)
    return np.concatenate([nominal[1:], np.zeros_like(nominal[:1])], axis=0)


def default_cost(beta: float = 0.0):
    """sum_t PE_reward + beta sum_t sum a^2 per sample: the field energy the reference rewards against (r_pe) and the
    control effort (r_ie)."""
    def cost(KE, PE, PE_reward, actions):
        return PE_reward.sum(axis=0) + beta * (np.asarray(actions) ** 2).sum(axis=(0, 2))
    return cost


def _plant_like(plant):
    """(constructor keywords of a BatchedPIC with the plant's physics, the plant's actuator)"""
    if hasattr(plant, "_like"):                       # BatchedPIC
        return dict(plant._like), plant._actuator
    like = dict(N=plant.N, N_mesh=plant.N_mesh, n0=plant.n0, L=plant.L, dt=plant.dt, gamma=plant.gamma, interpol=plant.interpol,
                device=plant.device, dtype=plant.dtype, position_dtype=plant.position_dtype, integrator=plant.integrator)
    return like, getattr(plant, "_actuator", None)


class MPPI:
    """Model-predictive path-integral control of `plant`: a BatchedPIC (its environment 0 is controlled; every environment
    is stepped under the same action) or a PIC, with an actuator set (`set_actuator`).

    samples: candidate sequences per plan (sample 0 is the nominal); horizon: steps each is rolled out; sigma: standard
    deviation of the perturbation of every coefficient; temperature: of the softmin weights; cost: None (`default_cost(beta)`)
    or a callable (KE, PE, PE_reward [horizon, samples], actions [horizon, samples, 2 max_mode]) -> [samples]; seed: of the
    generator the perturbations come from (same seed, same plant state: same actions)."""

    def __init__(self, plant, samples: int = 64, horizon: int = 10, sigma: float = 0.1, temperature: float = 1.0,
                 cost: Optional[Callable] = None, seed: int = 0, beta: float = 0.0, blocks_per_env: int = 0):
        from .batched import BatchedPIC
        like, actuator = _plant_like(plant)
        if actuator is None:
            raise ValueError("MPPI: the plant needs an actuator (set_actuator) before a planner is made for it")
        self.plant, self.samples, self.horizon = plant, int(samples), int(horizon)
        self.sigma, self.temperature = float(sigma), float(temperature)
        self.cost = default_cost(beta) if cost is None else cost
        self.rng = np.random.default_rng(seed)
        self.sim = BatchedPIC(self.samples, blocks_per_env=blocks_per_env, **like)
        self.sim.set_actuator(actuator)
        self.n_act = 2 * actuator.max_mode
        self.nominal = np.zeros((self.horizon, self.n_act))
        self.last_actions = self.last_history = self.last_costs = self.last_weights = None

    def plan(self):
        """One planning round from the plant's present state; returns the new nominal [horizon, 2 max_mode].  The plant is
        only read.  Kept for inspection: last_actions (what was rolled out), last_history (KE, PE, PE_reward of every step
        and sample), last_costs, last_weights."""
        self.sim.copy_from(self.plant, 0)
        actions = mppi_draw(self.nominal, self.samples, self.sigma, self.rng)
        hist = self.sim.step_actions_traj(actions, history=True)
        costs = np.asarray(self.cost(hist[0], hist[1], hist[2], actions), dtype=np.float64)
        weights = mppi_weights(costs, self.temperature)
        self.last_actions, self.last_history, self.last_costs, self.last_weights = actions, hist, costs, weights
        self.nominal = mppi_update(actions, weights)
        return self.nominal

    def act(self):
        """Step the plant under the nominal's first action, shift the nominal; returns that action [2 max_mode]."""
        a = self.nominal[0].copy()
        if hasattr(self.plant, "step_actions"):
            self.plant.step_actions(np.broadcast_to(a, (self.plant.num_envs, self.n_act)))
        else:
            self.plant.step(a)
        self.nominal = mppi_shift(self.nominal)
        return a

    def close(self):
        self.sim.close()
