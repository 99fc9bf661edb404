"""Shared case tables of the action-wrapper tests (ClipAction / RescaleAction / TransformAction) and a NumPy restatement of the two formulas.

tests/golden/make_golden_action_wrappers.py runs the REFERENCE's wrappers on these inputs and records what they forward;
tests/test_action_wrappers.py compares the restatement below and the package's NumPy path with that recording, bit for bit;
tests/test_gpu_action_wrappers.py -- on a machine without the reference -- compares the device kernel with the recording and, where a case has
no recorded counterpart (other batch sizes, the MuJoCo twins), with the restatement.
"""
import numpy as np

# name -> (action dimensions, symmetric bound): the Box shapes of Pendulum-v1, MountainCarContinuous-v0, Ant-v5, Humanoid-v5, Pusher-v5
BOXES = {"pendulum": (1, 2.0), "mountaincar_continuous": (1, 1.0), "ant": (8, 1.0), "humanoid": (17, 0.4), "pusher": (7, 2.0)}
# wrapper stacks recorded per box; the ones marked same have a batched space equal to the env's (the reference's `same_out`)
TRANSFORMS = ("clip", "rescale01", "rescale_pm1", "rescale_same", "clip01")
INPUTS = ("f32", "f64", "i64", "list", "list_int")
TRAJ_ENVS = {"pendulum": "Pendulum-v1", "mountaincar_continuous": "MountainCarContinuous-v0"}
TRAJ_WRAPPERS = ("clip", "rescale_pm1", "rescale_same", "clip_rescale_pm1")
TRAJ_N, TRAJ_T, TRAJ_SEED = 3, 40, 11
SAMPLE_SEED, SAMPLE_BATCHES, SAMPLE_N = 3, 10, 3
SAMPLE_BOXES = ("pendulum", "ant")


def make_box(spaces, name):
    dim, bound = BOXES[name]
    return spaces.Box(-bound, bound, shape=(dim,), dtype=np.float32)


class SpacesOnlyEnv:
    """A vector env that has nothing but spaces: what a wrapper's constructor and ``actions()`` look at."""

    metadata = {}

    def __init__(self, spaces, batch_space, single_action_space, num_envs):
        self.num_envs = num_envs
        self.single_action_space = single_action_space
        self.action_space = batch_space(single_action_space, num_envs)
        self.single_observation_space = spaces.Box(-1.0, 1.0, shape=(1,), dtype=np.float32)
        self.observation_space = batch_space(self.single_observation_space, num_envs)

    @property
    def unwrapped(self):
        return self


def build(wrappers, env, transform):
    """The wrapper stack ``transform`` names, from ``wrappers`` (the reference's gymnasium.wrappers.vector or gymnasium_amd.wrappers) over ``env``;
    returns the OUTERMOST wrapper (whose ``actions()`` the fixture records)."""
    box = env.single_action_space
    if transform == "clip":
        return wrappers.ClipAction(env)
    if transform == "rescale01":
        return wrappers.RescaleAction(env, 0.0, 1.0)
    if transform == "rescale_pm1":
        return wrappers.RescaleAction(env, -1.0, 1.0)
    if transform == "rescale_same":
        return wrappers.RescaleAction(env, box.low.copy(), box.high.copy())
    if transform == "clip01":  # ClipAction over RescaleAction(0, 1): clips to [0, 1], a ZERO bound
        return wrappers.ClipAction(wrappers.RescaleAction(env, 0.0, 1.0))
    if transform == "clip_rescale_pm1":
        return wrappers.ClipAction(wrappers.RescaleAction(env, -1.0, 1.0))
    raise KeyError(transform)


def special_values(bound):
    """float64 values around everything the two formulas treat specially, for a Box of +-bound (and the [0, 1] box of ``clip01``)."""
    b32 = float(np.float32(bound))  # the bound as the space holds it
    tiny = float(np.float32(1e-45))  # the smallest float32 denormal
    v = [0.0, -0.0, b32, -b32, 1.0, -1.0, 0.5 * bound, -0.25 * bound, 3.0 * bound, -3.0 * bound, np.inf, -np.inf, np.nan,
         tiny, -tiny, 3.0 * tiny, float(np.float32(1.1e-38)), -float(np.float32(1.1e-38)),
         float(np.nextafter(np.float32(b32), np.float32(np.inf))), float(np.nextafter(np.float32(b32), np.float32(0))),
         -float(np.nextafter(np.float32(b32), np.float32(np.inf))), -float(np.nextafter(np.float32(b32), np.float32(0))),
         # float64 values that round ACROSS a bound when stored as float32
         float(np.nextafter(b32, np.inf)), float(np.nextafter(b32, 0.0)), -float(np.nextafter(b32, np.inf)), -float(np.nextafter(b32, 0.0)),
         b32 * (1 + 1e-9), b32 * (1 - 1e-9), -b32 * (1 + 1e-9), -b32 * (1 - 1e-9), float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0)),
         1e-320, -1e-320, 1e300, -1e300, 1 / 3, -2 / 3]
    return np.array(v, dtype=np.float64)


def inputs(name):
    """The recorded input batches of one box: {input name: (N, A) array or nested list}; N is what the special values need at this width."""
    dim, bound = BOXES[name]
    rng = np.random.default_rng(100 + dim + int(bound * 10))
    sp = special_values(bound)
    rows = -(-(len(sp) + 8) // dim)
    flat = rng.uniform(-2.0 * bound, 2.0 * bound, rows * dim)
    flat[rng.permutation(rows * dim)[:len(sp)]] = sp  # the special values at scattered columns
    f64 = flat.reshape(rows, dim)
    i64 = rng.integers(-3, 4, (rows, dim))
    finite = np.where(np.isfinite(f64), f64, 0.25 * bound)  # (nested lists of Python floats: inf / NaN would not be exact Python literals in a case table)
    with np.errstate(over="ignore"):  # (+-1e300 become +-inf)
        f32 = f64.astype(np.float32)
    return {"f32": f32, "f64": f64, "i64": i64, "list": finite.tolist(), "list_int": i64.tolist()}


def tiled(arr, rows):
    """``rows`` rows cycling through the rows of ``arr``: every row is transformed on its own, so a recording tiles the same way."""
    arr = np.asarray(arr)
    return arr[np.arange(rows) % arr.shape[0]]


def trajectory_actions(env_name, dtype):
    """The [T, N, 1] action batches of the recorded trajectories: a third of the entries outside the WRAPPER's bounds (and so outside the env's)."""
    _, bound = BOXES[env_name]
    rng = np.random.default_rng(7 if dtype == np.float32 else 8)
    a = rng.uniform(-bound, bound, (TRAJ_T, TRAJ_N, 1))
    out = rng.random(a.shape) < 1 / 3
    a[out] = np.sign(a[out]) * rng.uniform(1.05, 3.0, int(out.sum())) * bound
    return a.astype(dtype)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def compute_dtype(a):
    """The dtype NumPy's promotion gives a row of ``a`` against float32 parameters."""
    return np.result_type(np.asarray(a).dtype, np.float32)


def clip(a, low, high, out_dtype=np.float32):
    """np.clip's loop restated: max(x, lo) = x > lo ? x : lo, min(t, hi) = t < hi ? t : hi, a NaN operand returned as it is; in the promoted
    dtype, rounded once to ``out_dtype``."""
    c = compute_dtype(a)
    x, lo, hi = np.asarray(a).astype(c), np.asarray(low).astype(c), np.asarray(high).astype(c)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(x), x, np.where(x > lo, x, lo))
        t = np.where(np.isnan(t), t, np.where(t < hi, t, hi))
    return t.astype(out_dtype)


def affine_inverse(a, intercept, gradient, out_dtype=np.float32):
    """(a - intercept) / gradient in the promoted dtype, rounded once to ``out_dtype``."""
    c = compute_dtype(a)
    with np.errstate(all="ignore"):
        return ((np.asarray(a).astype(c) - np.asarray(intercept).astype(c)) / np.asarray(gradient).astype(c)).astype(out_dtype)


def rescale_parameters(low, high, new_min, new_max):
    """(gradient, intercept) of rescale_box for float32 bounds and scalar or array targets, as float32 arrays."""
    low, high = np.asarray(low, np.float32), np.asarray(high, np.float32)
    new_min, new_max = (b if isinstance(b, np.ndarray) else np.full(low.shape, b) for b in (new_min, new_max))
    wide = getattr(np, "float128", np.float64)
    gradient = np.ones_like(new_min, dtype=np.float32)
    gradient[:] = (new_max - new_min) / (np.array(high, dtype=wide) - np.array(low, dtype=wide))
    intercept = np.zeros_like(new_min, dtype=np.float32)
    intercept[:] = gradient * -low + new_min
    return gradient, intercept


def restate(transform, name, a, same_dtype=None):
    """What the stack ``transform`` over box ``name`` forwards for the batch ``a`` (an array).  ``same_dtype``: the dtype a `same_out` stack keeps."""
    dim, bound = BOXES[name]
    low, high = np.full(dim, -bound, np.float32), np.full(dim, bound, np.float32)
    if transform == "clip":
        return clip(a, low, high)
    if transform == "clip01":
        return clip(a, np.zeros(dim, np.float32), np.ones(dim, np.float32))
    target = {"rescale01": (0.0, 1.0), "rescale_pm1": (-1.0, 1.0), "rescale_same": (low.copy(), high.copy())}[transform]
    g, i = rescale_parameters(low, high, *target)
    return affine_inverse(a, i, g, np.float32 if same_dtype is None else same_dtype)


def is_same_out(transform, name):
    return transform == "rescale_same" or (transform == "rescale_pm1" and BOXES[name][1] == 1.0)


def bits(a):
    """An integer view for bit-for-bit comparison (NaN compares by its bits as well: the formulas return the caller's NaN)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} != {want.dtype} {want.shape}"
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN at other positions"
    bad = (bits(got) != bits(want)) & ~nan_w
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at {np.argwhere(bad)[0]}: {got[bad][0]!r} != {want[bad][0]!r}"
