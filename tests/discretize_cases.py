"""The inputs of tests/golden/discretize.npz (tests/golden/make_golden_discretize.py records the reference's answers to them) and what
tests/test_discretize.py and tests/test_gpu_discretize.py share.  NumPy only; the crafted inputs are stored in the fixture beside the answers, so the
tests never rebuild them."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "discretize.npz")

F32, F64 = np.float32, np.float64
# name -> (low, high, dtype)
BOXES = {
    "pendulum": ([-1.0, -1.0, -8.0], [1.0, 1.0, 8.0], F32),
    "mountaincar": ([-1.2, -0.07], [0.6, 0.07], F32),  # (high - 1e-8 equals high for 0.6 and differs for 0.07)
    "acrobot": ([-1.0, -1.0, -1.0, -1.0, -12.566371, -28.274334], [1.0, 1.0, 1.0, 1.0, 12.566371, 28.274334], F32),
    "one": ([-2.0], [2.0], F32),
    "duplicate": ([-1.0, 0.5, 0.0], [1.0, 0.5, 0.0], F32),  # low == high in two components: duplicate edges, one with high - 1e-8 below low
    "wide64": ([-1.2, -0.07, -3.0], [0.6, 0.07, 5.0], F64),
    "hopper": ([-1.0] * 3, [1.0] * 3, F32),
    "ant": ([-1.0] * 8, [1.0] * 8, F32),
    "humanoid": ([-0.4] * 17, [0.4] * 17, F32),
    "act64": ([-1.0, -0.5, 0.0], [1.0, 0.25, 3.0], F64),
}
MAX_TABLE = 2048  # MI_DISCRETIZE_MAX_TABLE
# case -> (box, bins, multidiscrete)
OBS_CASES = {
    "pendulum_345": ("pendulum", (3, 4, 5), False),
    "pendulum_345_multi": ("pendulum", (3, 4, 5), True),
    "pendulum_1": ("pendulum", 1, False),
    "pendulum_10": ("pendulum", 10, False),
    "mountaincar_2": ("mountaincar", 2, False),
    "mountaincar_10_multi": ("mountaincar", 10, True),
    "acrobot_3": ("acrobot", 3, False),
    "acrobot_mixed_multi": ("acrobot", (2, 1, 3, 4, 5, 6), True),
    "one_257": ("one", 257, False),
    "one_257_multi": ("one", (257,), True),
    "one_cap": ("one", MAX_TABLE + 1, False),  # a table AT the LDS cap
    "duplicate_4": ("duplicate", 4, False),
    "duplicate_4_multi": ("duplicate", 4, True),
    "wide64_345": ("wide64", (3, 4, 5), False),
    "wide64_345_multi": ("wide64", (3, 4, 5), True),
}
ACT_CASES = {
    "one_7": ("one", 7, False),
    "one_7_multi": ("one", 7, True),
    "hopper_345": ("hopper", (3, 4, 5), False),
    "hopper_315": ("hopper", (3, 1, 5), False),
    "hopper_315_multi": ("hopper", (3, 1, 5), True),
    "ant_3": ("ant", 3, False),  # prod = 6561: the 32-bit path for indices in [0, 2^31)
    "ant_17": ("ant", 17, False),  # prod = 17^8 > 2^31: the 64-bit path for every index
    "ant_5_multi": ("ant", 5, True),
    "humanoid_2": ("humanoid", 2, False),
    "humanoid_4": ("humanoid", 4, False),  # prod = 2^34
    "humanoid_mixed_multi": ("humanoid", tuple(1 + (k % 5) for k in range(17)), True),
    "act64_345": ("act64", (3, 4, 5), False),
    "act64_345_multi": ("act64", (3, 4, 5), True),
}
# refused constructor calls: name -> (wrapper, env id or box name, bins)
REFUSED = {
    "obs_cartpole": ("obs", "CartPole-v1", 4),
    "obs_mujoco": ("obs", "HalfCheetah-v5", 4),
    "obs_discrete": ("obs", "FrozenLake-v1", 4),
    "obs_bins_length": ("obs", "Pendulum-v1", (3, 4)),
    "act_discrete": ("act", "CartPole-v1", 4),
    "act_bins_length": ("act", "Pendulum-v1", (3, 4)),
}
SAMPLE_CASES = {"flat": ("Pendulum-v1", 7, False), "multi": ("MountainCarContinuous-v0", (5,), True)}
SAMPLE_SEED, SAMPLE_N, SAMPLE_BATCHES = 11, 5, 3

# trajectories: name -> (env id, obs (bins, multidiscrete) or None, act (bins, multidiscrete) or None, FlattenObservation on top)
TRAJ = {
    "pendulum_flat": ("Pendulum-v1", ((3, 4, 5), False), (7, False), False),
    "pendulum_multi": ("Pendulum-v1", (4, True), (5, True), False),
    "acrobot_flat": ("Acrobot-v1", (3, False), None, False),
    "mountaincar_onehot": ("MountainCar-v0", (4, False), None, True),
    "mountaincar_continuous_multi": ("MountainCarContinuous-v0", ((5, 6), True), ((4,), True), False),
}
MODES = ("next", "same", "disabled")
# (the vector FlattenObservation refuses SAME_STEP like the reference's: that stack is compared in the two other modes)
TRAJ_KEYS = [(name, mode) for name in TRAJ for mode in MODES if not (TRAJ[name][3] and mode == "same")]
N, T, SEED, ASEED, LIMIT, MASK_AT = 3, 10, 7, 5, 4, 5
MASK = np.array([True, False, True])


def box_arrays(name):
    low, high, dtype = BOXES[name]
    return np.array(low, dtype=dtype), np.array(high, dtype=dtype)


def bins_array(name, bins):
    n = len(BOXES[name][0])
    return np.array([bins] * n if isinstance(bins, int) else bins)


def obs_inputs(name, bins):
    """Rows of observations around everything the discretization compares against: per dimension the bounds, the clip bound, every edge and its two
    float neighbours, values beyond both bounds, +-inf, NaN and -0.0 -- each placed in an otherwise ordinary row -- and a few rows of extremes."""
    low, high = box_arrays(name)
    dtype, b = low.dtype, bins_array(name, bins)
    base = (low + dtype.type(0.37) * (high - low)).astype(dtype)
    rows = [base, low, high, np.full_like(low, np.nan), np.full_like(low, np.inf), np.full_like(low, -np.inf), (high - 1e-8).astype(dtype)]
    for d in range(len(low)):
        edges = np.linspace(low[d], high[d], b[d] + 1).astype(dtype)  # (the bounds are edges 0 and bins)
        special = np.concatenate([edges, np.nextafter(edges, dtype.type(-np.inf)), np.nextafter(edges, dtype.type(np.inf)),
                                  np.array([high[d] - 1e-8, low[d] - 1, high[d] + 1, low[d] * 3 - 1, np.inf, -np.inf, np.nan, -0.0, 0.0], dtype=dtype)])
        for v in special:
            row = base.copy()
            row[d] = v
            rows.append(row)
    return np.stack(rows).astype(dtype)


def act_inputs(name, bins, multidiscrete):
    """Index batches: every valid index where there are few, a spread of them otherwise, and the out-of-range ones -- flat: -1, -prod, prod, prod + 1
    and indices beyond +-2^31 (floor % and //: they wrap); multidiscrete: below 0 and above bins - 1 (they clamp)."""
    b = bins_array(name, bins).astype(np.int64)
    rng = np.random.default_rng(3)
    if not multidiscrete:
        prod = int(np.prod([int(x) for x in b], dtype=object))
        valid = np.arange(prod) if prod <= 600 else np.unique(np.concatenate([np.arange(40), prod - 1 - np.arange(40), rng.integers(0, prod, 200)]))
        extra = [-1, -2, -prod, -prod - 1, prod, prod + 1, 3 * prod + 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5, -2 ** 31, -2 ** 31 - 1, -2 ** 31 - 7,
                 2 ** 40 + 3, -2 ** 40 - 3, 2 ** 62 + 11, -2 ** 62 - 11]
        return np.concatenate([valid, np.array(extra, dtype=np.int64)]).astype(np.int64)
    rows = [rng.integers(0, b) for _ in range(60)] + [np.zeros_like(b), b - 1, b, -np.ones_like(b), b + 3, np.full_like(b, -2 ** 40), np.full_like(b, 2 ** 33)]
    for d in range(len(b)):
        for v in (-1, -7, 0, int(b[d]) - 1, int(b[d]), int(b[d]) + 2, 2 ** 31 + 1, -2 ** 31 - 1):
            row = rng.integers(0, b)
            row[d] = v
            rows.append(row)
    return np.stack(rows).astype(np.int64)


def wrap(w, env, name):
    """The stack of TRAJ[name] over ``env``; ``w``: a module with DiscretizeObservation, DiscretizeAction, FlattenObservation (gymnasium.wrappers for a
    scalar env, gymnasium_amd.wrappers for a vector env)."""
    _, obs, act, flatten = TRAJ[name]
    if obs is not None:
        env = w.DiscretizeObservation(env, obs[0], multidiscrete=obs[1])
    if act is not None:
        env = w.DiscretizeAction(env, act[0], multidiscrete=act[1])
    if flatten:
        env = w.FlattenObservation(env)
    return env


class SpacesOnlyEnv:
    """A vector env that has only spaces: enough for the wrappers' constructors and ``observations()`` / ``actions()``."""

    def __init__(self, obs_space, act_space, num_envs):
        from gymnasium_amd.gym_api import AutoresetMode, batch_space

        self.metadata = {"autoreset_mode": AutoresetMode.NEXT_STEP}
        self.num_envs = num_envs
        self.single_observation_space, self.single_action_space = obs_space, act_space
        self.observation_space, self.action_space = batch_space(obs_space, num_envs), batch_space(act_space, num_envs)
        self.unwrapped = self


def box_of(name):
    from gymnasium_amd.gym_api import spaces

    low, high = box_arrays(name)
    return spaces.Box(low, high, dtype=low.dtype)


def obs_wrapper(case, rows=3):
    """gymnasium_amd's DiscretizeObservation of OBS_CASES[case] over a spaces-only env of ``rows`` sub-environments."""
    from gymnasium_amd import wrappers
    from gymnasium_amd.gym_api import spaces

    name, bins, multi = OBS_CASES[case]
    return wrappers.DiscretizeObservation(SpacesOnlyEnv(box_of(name), spaces.Discrete(2), rows), bins, multidiscrete=multi)


def act_wrapper(case, rows=3):
    from gymnasium_amd import wrappers
    from gymnasium_amd.gym_api import spaces

    name, bins, multi = ACT_CASES[case]
    return wrappers.DiscretizeAction(SpacesOnlyEnv(spaces.Discrete(2), box_of(name), rows), bins, multidiscrete=multi)


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _FIX = {k: z[k] for k in z.files}
    return _FIX


def errors():
    return dict(e.split("=") for e in fixture()["errors"])


def tiled(x, rows):
    """``rows`` rows out of a recording, repeated as often as needed (the rows of a batch are independent)."""
    return x[np.arange(rows) % len(x)]
