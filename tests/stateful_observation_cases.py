"""NumPy restatement of gymnasium.wrappers.FrameStackObservation / DelayObservation / TimeAwareObservation around every scalar env of a
SyncVectorEnv, vectorised over the sub-environments (wrappers/stateful_observation.py:35-103, 106-301, 304-461, vector/sync_vector_env.py:207-337).

The wrappers move data (plus one division for the normalised time), so the restatement is written the way the REFERENCE keeps its state -- a rolling
stack, a queue that pops, a counter -- and not the way the kernels decide their sources (gymnasium_amd/csrc/stateful_observation_internal.h):
tests/test_stateful_observation_host.py pins it to the fixtures recorded from the reference (array_equal) and compares the header, compiled for the
host, with it; the GPU tests then lean on it where no fixture exists (other batch sizes, MuJoCo, RepeatAction underneath).

A layer has ``reset_rows(x, rows)`` and ``step_rows(x, rows)``: the scalar wrappers' ``reset()`` / ``step()`` of the rows in the bool mask, given the
full input batch; both return the full output batch as the vector env holds it afterwards (the other rows keep what they returned last).
"""
import os

import numpy as np

import per_env_normalize_cases as normalize_cases

IDS = {"cartpole": "CartPole-v1", "pendulum": "Pendulum-v1", "mountaincar": "MountainCar-v0"}
# cartpole: long enough to fall over before the limit (terminations that are no truncations), t / 14; pendulum: 3 observations per episode, fewer
# than the largest stack holds; mountaincar: exactly the 4 observations of the largest stack, a queue of delay 3 that pops once per episode, t / 3
LIMITS = {"cartpole": 14, "pendulum": 2, "mountaincar": 3}
CUSTOM = {"cartpole": np.array([0.5, -1.0, 0.25, 2.0], np.float32), "pendulum": np.array([0.5, -0.5, 1.5], np.float32),
          "mountaincar": np.array([-0.7, 0.03], np.float32)}
MODES = ("next", "same", "disabled")
N, T, SEED, ASEED = 70, 40, 3, 1
KMAX = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> the layers from the innermost to the outermost: (kind, keyword arguments)
CONFIGS = {}
for _k in (1, 3, 4):
    for _p in ("reset", "zero", "custom"):
        CONFIGS[f"stack{_k}_{_p}"] = [("stack", dict(k=_k, padding=_p))]
for _d in (0, 1, 3):
    CONFIGS[f"delay{_d}"] = [("delay", dict(delay=_d))]
CONFIGS["time_int"] = [("time", dict(flatten=True, normalize_time=False))]
CONFIGS["time_normalized"] = [("time", dict(flatten=True, normalize_time=True))]
CONFIGS["time_dict"] = [("time", dict(flatten=False, normalize_time=False))]
CONFIGS["chain_stack_time_delay"] = [("delay", dict(delay=1)), ("time", dict(flatten=True, normalize_time=False)), ("stack", dict(k=3, padding="reset"))]
CONFIGS["chain_stack_normalize"] = [("normalize", dict()), ("stack", dict(k=3, padding="zero"))]


def pack(arrays):
    """name -> array as the two members of a fixture file: every array's bytes in ONE stream (``blob``) behind a directory (``names``: one
    "name;dtype;shape" entry per array, in order)."""
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    names = np.array([f"{k};{v.dtype.str};{','.join(map(str, v.shape))}" for k, v in arrays.items()])
    blob = np.frombuffer(b"".join(v.tobytes() for v in arrays.values()), dtype=np.uint8)
    return {"names": names, "blob": blob}


def load(path):
    with np.load(path, allow_pickle=False) as z:
        names, blob = z["names"], z["blob"]
    out, at = {}, 0
    for entry in names.tolist():
        name, dtype, shape = entry.split(";")
        shape = tuple(int(s) for s in shape.split(",")) if shape else ()
        size = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        out[name] = np.frombuffer(blob[at:at + size].tobytes(), dtype=np.dtype(dtype)).reshape(shape)
        at += size
    assert at == blob.size
    return out


_FIXTURES = {}


def fixture(key):
    """The arrays of stateful_observation_<key>.npz (read-only, loaded once)."""
    if key not in _FIXTURES:
        _FIXTURES[key] = load(os.path.join(GOLDEN, f"stateful_observation_{key}.npz"))
    return _FIXTURES[key]


class _Layer:
    def __init__(self, num_envs, shape, dtype):
        self.n, self.in_shape, self.in_dtype = num_envs, tuple(shape), np.dtype(dtype)

    def _emit(self, out, rows):
        self.last[rows] = out[rows]
        return self.last.copy()


class FrameStack(_Layer):
    def __init__(self, num_envs, shape, dtype, k, padding="reset", custom=None):
        super().__init__(num_envs, shape, dtype)
        self.k, self.padding = k, padding
        self.custom = None if custom is None else np.asarray(custom, dtype=dtype).reshape(shape)
        self.out_shape, self.out_dtype = (k,) + self.in_shape, self.in_dtype
        self.stack = np.zeros((num_envs,) + self.out_shape, self.in_dtype)  # obs_queue, oldest first
        self.last = self.stack.copy()

    def reset_rows(self, x, rows):
        x = np.asarray(x, self.in_dtype).reshape((self.n,) + self.in_shape)
        pad = x if self.padding == "reset" else (np.zeros_like(x) if self.padding == "zero" else np.broadcast_to(self.custom, x.shape))
        for _ in range(self.k - 1):
            self.stack[rows] = np.concatenate([self.stack[:, 1:], pad[:, None]], axis=1)[rows]
        return self.step_rows(x, rows)

    def step_rows(self, x, rows):
        x = np.asarray(x, self.in_dtype).reshape((self.n,) + self.in_shape)
        self.stack[rows] = np.concatenate([self.stack[:, 1:], x[:, None]], axis=1)[rows]
        return self._emit(self.stack, rows)


class Delay(_Layer):
    def __init__(self, num_envs, shape, dtype, delay):
        super().__init__(num_envs, shape, dtype)
        self.delay = delay
        self.out_shape, self.out_dtype = self.in_shape, self.in_dtype
        self.queue = np.zeros((num_envs, delay + 1) + self.in_shape, self.in_dtype)  # the last `length` slots are the queue, oldest first
        self.length = np.zeros(num_envs, np.int64)
        self.last = np.zeros((num_envs,) + self.in_shape, self.in_dtype)

    def reset_rows(self, x, rows):
        self.length[rows] = 0
        return self.step_rows(x, rows)

    def step_rows(self, x, rows):
        x = np.asarray(x, self.in_dtype).reshape((self.n,) + self.in_shape)
        self.queue[rows] = np.concatenate([self.queue[:, 1:], x[:, None]], axis=1)[rows]
        self.length[rows] += 1
        pops = rows & (self.length > self.delay)
        out = np.zeros_like(self.last)
        out[pops] = self.queue[pops, 0]
        self.length[pops] -= 1
        return self._emit(out, rows)


class TimeAware(_Layer):
    def __init__(self, num_envs, shape, dtype, max_timesteps, flatten=True, normalize_time=False):
        super().__init__(num_envs, shape, dtype)
        self.flatten, self.normalize_time, self.max_timesteps = flatten, normalize_time, max_timesteps
        self.time_dtype = np.dtype(np.float32 if normalize_time else np.int32)
        dim = int(np.prod(shape))
        self.out_shape = (dim + 1,) if flatten else (1,)
        self.out_dtype = np.result_type(self.in_dtype, self.time_dtype) if flatten else self.time_dtype
        self.timesteps = np.zeros(num_envs, np.int64)
        self.last = np.zeros((num_envs,) + self.out_shape, self.out_dtype)

    def _observation(self, x, rows):
        x = np.asarray(x, self.in_dtype).reshape(self.n, -1)
        if self.normalize_time:
            time = np.array([t / self.max_timesteps for t in self.timesteps.tolist()], dtype=np.float32)  # Python's true division, rounded once more
        else:
            time = self.timesteps.astype(np.int32)
        out = np.concatenate([x.astype(self.out_dtype), time[:, None].astype(self.out_dtype)], axis=1) if self.flatten else time[:, None]
        return self._emit(out, rows)

    def reset_rows(self, x, rows):
        self.timesteps[rows] = 0
        return self._observation(x, rows)

    def step_rows(self, x, rows):
        self.timesteps[rows] += 1
        return self._observation(x, rows)


class Normalize(_Layer):
    """per_env.NormalizeObservation underneath: the restatement of tests/per_env_normalize_cases.py."""

    def __init__(self, num_envs, shape, dtype):
        super().__init__(num_envs, shape, dtype)
        self.impl = normalize_cases.ObsNormalizer(num_envs, int(np.prod(shape)), dtype)
        self.out_shape, self.out_dtype = self.in_shape, np.dtype(np.float32)

    def reset_rows(self, x, rows):
        return self.impl.observe(np.asarray(x).reshape(self.n, -1), rows).reshape((self.n,) + self.in_shape)

    step_rows = reset_rows


def build(layers, num_envs, shape, dtype, max_timesteps, custom=None):
    """The restatement objects of a configuration, innermost first."""
    out = []
    for kind, kw in layers:
        if kind == "stack":
            layer = FrameStack(num_envs, shape, dtype, kw["k"], kw["padding"], custom if kw["padding"] == "custom" else None)
        elif kind == "delay":
            layer = Delay(num_envs, shape, dtype, kw["delay"])
        elif kind == "time":
            layer = TimeAware(num_envs, shape, dtype, max_timesteps, kw["flatten"], kw["normalize_time"])
        else:
            layer = Normalize(num_envs, shape, dtype)
        out.append(layer)
        shape, dtype = layer.out_shape, layer.out_dtype
    return out


class Stack:
    """A chain of layers as one: what SyncVectorEnv over the wrapped scalar envs does with the rows of a call."""

    def __init__(self, layers, mode):
        self.layers, self.mode = layers, mode
        self.pending = np.zeros(layers[0].n, dtype=bool)

    def _through(self, method, x, rows):
        for layer in self.layers:
            x = getattr(layer, method)(x, rows)
        return x

    def reset(self, x, rows=None):
        rows = np.ones(self.layers[0].n, dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
        self.pending &= ~rows
        return self._through("reset_rows", x, rows)

    def step(self, x, terminated, truncated, final_obs=None, final_mask=None):
        """The outputs of one vector step; under SAME_STEP also the outputs for the final observations (zeros outside the mask)."""
        done = np.asarray(terminated, dtype=bool) | np.asarray(truncated, dtype=bool)
        every = np.ones(len(done), dtype=bool)
        if self.mode == "same":
            fm = np.zeros(len(done), dtype=bool) if final_mask is None else np.asarray(final_mask, dtype=bool)
            fin = None
            if fm.any():
                fin = self._through("step_rows", final_obs, fm)
                fin = np.where(fm.reshape((-1,) + (1,) * (fin.ndim - 1)), fin, np.zeros_like(fin))
                self._through("reset_rows", x, fm)
            return self._through("step_rows", x, ~fm), fin
        if self.mode == "next":
            if self.pending.any():
                self._through("reset_rows", x, self.pending)
            out = self._through("step_rows", x, ~self.pending)
            self.pending = done
            return out, None
        self.pending = done
        return self._through("step_rows", x, every), None


def replay(fix, mode, layers):
    """The recorded unwrapped trajectory of a fixture through a configuration: obs0, obs [T, ...], final_obs / reset_obs where the mode has them."""
    stack = Stack(layers, mode)
    out = {"obs0": stack.reset(fix["obs0"]), "obs": [], "final_obs": [], "reset_obs": []}
    steps = len(fix["obs"])
    for t in range(steps):
        fm = fix["final_mask"][t] if mode == "same" else None
        o, fin = stack.step(fix["obs"][t], fix["term"][t], fix["trunc"][t], fix["final_obs"][t] if mode == "same" else None, fm)
        out["obs"].append(o)
        if mode == "same":
            out["final_obs"].append(np.zeros_like(o) if fin is None else fin)
        if mode == "disabled":
            ro = np.zeros_like(o)
            if fix["reset_mask"][t].any():
                ro = stack.reset(fix["reset_obs"][t], fix["reset_mask"][t])
            out["reset_obs"].append(ro)
    for k in ("obs", "final_obs", "reset_obs"):
        out[k] = np.stack(out[k]) if out[k] else None
    out["stack"] = stack
    return out


def rollout(stack, obs, term, trunc):
    """T steps of a NEXT_STEP / DISABLED env through a Stack that already carries state: [T, N, ...]."""
    return np.stack([stack.step(obs[t], term[t], trunc[t])[0] for t in range(len(obs))])


def wrap(env, key, layers):
    """The per_env wrappers of a configuration around a gymnasium_amd vector env (key: whose custom padding)."""
    from gymnasium_amd.wrappers import per_env

    for kind, kw in layers:
        if kind == "stack":
            env = per_env.FrameStackObservation(env, kw["k"], padding_type=CUSTOM[key] if kw["padding"] == "custom" else kw["padding"])
        elif kind == "delay":
            env = per_env.DelayObservation(env, kw["delay"])
        elif kind == "time":
            env = per_env.TimeAwareObservation(env, flatten=kw["flatten"], normalize_time=kw["normalize_time"])
        else:
            env = per_env.NormalizeObservation(env)
    return env
