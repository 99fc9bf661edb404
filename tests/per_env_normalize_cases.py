"""NumPy restatement of gymnasium.wrappers.NormalizeObservation / NormalizeReward around every scalar env of a SyncVectorEnv, vectorised over the
sub-environments (wrappers/stateful_observation.py:464-561, stateful_reward.py:20-142, wrappers/utils.py:33-71, vector/sync_vector_env.py:266-337).

Every expression below is ONE NumPy ufunc call per line of gymnasium_amd/csrc/per_env_normalize_internal.h, on arrays of the dtype the reference
computes in, so every operation is rounded once in that dtype.  tests/test_per_env_normalize_host.py pins it to the fixtures recorded from the
reference (array_equal); the GPU tests then lean on it where no fixture exists (Acrobot, MuJoCo, ToyText, RepeatAction / StickyAction underneath).
"""
import os

import numpy as np

IDS = {"cartpole": "CartPole-v1", "pendulum": "Pendulum-v1", "mountaincar_continuous": "MountainCarContinuous-v0"}
LIMITS = {"cartpole": 30, "pendulum": 7, "mountaincar_continuous": 25}
MODES = ("next", "same", "disabled")
N, T, GAMMA, SEED, ASEED = 70, 80, 0.99, 3, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(key):
    return np.load(os.path.join(GOLDEN, f"per_env_normalize_{key}.npz"), allow_pickle=False)


class ObsNormalizer:
    """NormalizeObservation of ``num_envs`` scalar envs: ``mean`` / ``var`` [N, D] in the observations' dtype, ``count`` [N] float64."""

    def __init__(self, num_envs, dim, dtype, epsilon=1e-8):
        self.dtype = np.dtype(dtype)
        assert self.dtype in (np.float32, np.float64)
        self.mean, self.var = np.zeros((num_envs, dim), self.dtype), np.ones((num_envs, dim), self.dtype)
        self.count = np.full(num_envs, 1e-4)
        self.first = np.ones(num_envs, dtype=bool)  # float64 only: the reference's arrays are float32 until the first update
        self.epsilon, self.update_running_mean = epsilon, True
        self.last = np.zeros((num_envs, dim), np.float32)

    def _update(self, x, rows):
        m, v, c = self.mean[rows], self.var[rows], self.count[rows]
        tot = c + 1.0
        d = x - m
        if self.dtype == np.float32:
            cf, tf = c.astype(np.float32)[:, None], tot.astype(np.float32)[:, None]
            ma = v * cf
        else:
            cf, tf = c[:, None], tot[:, None]
            quirk = (v.astype(np.float32) * c.astype(np.float32)[:, None]).astype(np.float64)
            ma = np.where(self.first[rows][:, None], quirk, v * cf)
        q = d / tf
        sq = d * d
        sc = sq * cf
        mc = sc / tf
        m2 = ma + mc
        self.mean[rows], self.var[rows], self.count[rows] = m + q, m2 / tf, tot
        self.first[rows] = False

    def observe(self, x, rows=None):
        """``observation()`` of the rows in ``rows`` (bool [N]; None: all); the full batch as the vector env holds it afterwards."""
        x = np.asarray(x, dtype=self.dtype)
        rows = np.ones(len(x), dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
        if self.update_running_mean:
            self._update(x[rows], rows)
        eps = np.float32(self.epsilon) if self.dtype == np.float32 else self.epsilon
        c = x[rows] - self.mean[rows]
        s = np.sqrt(self.var[rows] + eps)
        self.last = self.last.copy()
        self.last[rows] = (c / s).astype(np.float32)
        return self.last


class RewardNormalizer:
    """NormalizeReward of ``num_envs`` scalar envs under a vector env's autoreset ``mode`` ("next" / "same" / "disabled")."""

    def __init__(self, num_envs, gamma=0.99, epsilon=1e-8, mode="next"):
        self.acc, self.mean, self.var, self.count = np.zeros(num_envs), np.zeros(num_envs), np.ones(num_envs), np.full(num_envs, 1e-4)
        self.was_done = np.zeros(num_envs, dtype=bool)
        self.gamma, self.epsilon, self.mode, self.update_running_mean = gamma, epsilon, mode, True

    def reset(self, rows=None):
        if rows is None:
            self.was_done[:] = False
        else:
            self.was_done[np.asarray(rows, dtype=bool)] = False

    def step(self, reward, terminated, truncated):
        reward, terminated = np.asarray(reward, dtype=np.float64), np.asarray(terminated, dtype=bool)
        live = ~self.was_done if self.mode == "next" else np.ones(len(reward), dtype=bool)  # the rows whose scalar env really takes the step
        g = self.acc[live] * self.gamma
        k = g * (1 - terminated[live])
        self.acc[live] = k + reward[live]
        if self.update_running_mean:
            m, v, c, x = self.mean[live], self.var[live], self.count[live], self.acc[live]
            tot = c + 1.0
            d = x - m
            q = d / tot
            ma = v * c
            sq = d * d
            sc = sq * c
            mc = sc / tot
            m2 = ma + mc
            self.mean[live], self.var[live], self.count[live] = m + q, m2 / tot, tot
        out = np.zeros(len(reward))
        out[live] = reward[live] / np.sqrt(self.var[live] + self.epsilon)
        self.was_done = terminated | np.asarray(truncated, dtype=bool)
        return out


def replay(fix, mode, dtype=np.float32, gamma=GAMMA, epsilon=1e-8, reward=True, obs_cls=None, reward_cls=None):
    """The fixture's raw stream (raw_obs0, raw_obs, raw_reward, term, trunc, raw_final_obs / final_mask, reset_mask / raw_reset_obs) through the
    restatement: dict(obs0, obs, reward, final_obs, reset_obs, on, rn) with the normalisers as they stand after the last step.  ``obs_cls`` /
    ``reward_cls``: other implementations with the interface of ObsNormalizer / RewardNormalizer (the arithmetic header behind ctypes)."""
    raw_obs = fix["raw_obs"]
    steps, n, dim = raw_obs.shape
    on = (obs_cls or ObsNormalizer)(n, dim, dtype, epsilon)
    rn = (reward_cls or RewardNormalizer)(n, gamma, epsilon, mode) if reward else None
    out = {"obs0": on.observe(fix["raw_obs0"]), "obs": [], "reward": [], "final_obs": [], "reset_obs": []}
    for t in range(steps):
        if mode == "same":
            fm = fix["final_mask"][t]
            fo = np.zeros((n, dim), np.float32)
            if fm.any():
                fo[fm] = on.observe(fix["raw_final_obs"][t], fm)[fm]
            out["final_obs"].append(fo)
        out["obs"].append(on.observe(raw_obs[t]))
        if rn is not None:
            out["reward"].append(rn.step(fix["raw_reward"][t], fix["term"][t], fix["trunc"][t]))
        if mode == "disabled":
            rm = fix["reset_mask"][t]
            if rm.any():
                out["reset_obs"].append(on.observe(fix["raw_reset_obs"][t], rm))
                if rn is not None:
                    rn.reset(rm)
            else:
                out["reset_obs"].append(np.zeros((n, dim), np.float32))
    res = {k: (np.stack(v) if isinstance(v, list) and v else v) for k, v in out.items()}
    res["on"], res["rn"] = on, rn
    return res
