"""-m gpu: RescaleObservation / DtypeObservation / FlattenObservation / TransformObservation / TransformReward with device tensors
(mi_transform_observations, mi_one_hot; gymnasium_amd/csrc/observation_wrappers.hip).

The kernels are compared bit for bit (integer views, NaN by position) with what the REFERENCE's wrappers returned
(tests/golden/observation_wrappers.npz; rows are transformed independently, so a recording tiles to any batch size) and, where no recording exists,
with the NumPy restatement of tests/observation_wrapper_cases.py, which tests/test_observation_wrappers.py pins on the same recording.
"""
import ctypes as C

import numpy as np
import pytest

import observation_wrapper_cases as oc
import gymnasium_amd
from conftest import golden
from gymnasium_amd import _native
from gymnasium_amd import wrappers as gw
from gymnasium_amd.gym_api import AutoresetMode, batch_space, error, spaces

pytestmark = pytest.mark.gpu
BY_WIDTH = {2: "mountaincar", 3: "pendulum", 4: "cartpole", 6: "acrobot"}
MODES = {"NEXT_STEP": "NextStep", "DISABLED": "Disabled"}


@pytest.fixture(scope="module")
def gold():
    return golden("observation_wrappers.npz")


@pytest.fixture(scope="module")
def errors(gold):
    return dict(str(e).split("=", 1) for e in gold["errors"])


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stand_in(space, rows):
    return oc.SpacesOnlyEnv(spaces, batch_space, space, rows, AutoresetMode.NEXT_STEP)


def _code(dtype):
    import torch

    return {torch.float16: _native.MI_F16, torch.float32: _native.MI_F32, torch.float64: _native.MI_F64, torch.int32: _native.MI_I32,
            torch.int64: _native.MI_I64, torch.uint8: _native.MI_U8}[dtype]


def run_kernel(x, out, kind, dim=1, gradient=None, intercept=None):
    """mi_transform_observations on torch's current stream; ``x`` / ``out``: device tensors (views allowed) of the same number of elements."""
    import torch

    lib = _native.load_library()
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel()
    lib.check(lib.transform_observations(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(x.data_ptr()), _code(x.dtype),
                                         C.c_void_p(out.data_ptr()), _code(out.dtype), x.numel(), dim, kind,
                                         None if gradient is None else C.c_void_p(gradient.data_ptr()),
                                         None if intercept is None else C.c_void_p(intercept.data_ptr())))
    return out


def run_one_hot(parts, widths, out, starts=None):
    import torch

    lib = _native.load_library()
    k = len(parts)
    starts = [0] * k if starts is None else starts
    lib.check(lib.one_hot(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), (C.c_void_p * k)(*[p.data_ptr() for p in parts]), k,
                          (C.c_int64 * k)(*starts), (C.c_int32 * k)(*widths), parts[0].numel(), C.c_void_p(out.data_ptr())))
    return out


@pytest.mark.parametrize("rows", [1, 3, 64, 257])
@pytest.mark.parametrize("width", list(BY_WIDTH))
def test_rescale_and_dtype_equal_the_reference_recording(gold, errors, width, rows):
    """Bodies with and without head and tail: 1 x 2 elements (no group) up to 257 x 6, float32 boxes of every width."""
    name = BY_WIDTH[width]
    x = oc.crafted(name)
    given = oc.tiled(x, rows)
    for target in oc.RESCALE_TARGETS:
        key = f"r/{name}/{target}"
        if key in errors:
            continue
        w = oc.build(gw, stand_in(oc.make_box(spaces, name), rows), "rescale", target, name)
        t = _cuda(given)
        got = w.observations(t)
        assert got.is_cuda and got.data_ptr() != t.data_ptr()
        oc.assert_same_bits(_np(got), oc.tiled(gold[f"{key}/out"], rows), f"{key} rows={rows}")
        oc.assert_same_bits(_np(t), given, "the caller's tensor")
    for target in oc.DTYPE_TARGETS:
        key = f"d/{name}/{target}"
        if key in errors:
            continue
        w = oc.build(gw, stand_in(oc.make_box(spaces, name), rows), "dtype", target)
        batch = oc.tiled(oc.dtype_batch(name, target), rows)
        t = _cuda(batch)
        oc.assert_same_bits(_np(w.observations(t)), oc.tiled(gold[f"{key}/out"], rows), f"{key} rows={rows}")
        oc.assert_same_bits(_np(t), batch, "the caller's tensor")


@pytest.mark.parametrize("name", ["wide64", "level64", "level32", "frozenlake", "cliffwalking", "taxi"])
def test_every_cast_pair_equals_the_reference_recording(gold, errors, name):
    """float64 (-> float16 rounded once, -> float32), float32 and int64 sources to every target; a pair the reference's Box refuses at construction
    (an unsigned target) goes to the kernel directly, against NumPy's cast."""
    import torch

    for target in oc.DTYPE_TARGETS:
        key = f"d/{name}/{target}"
        if name in oc.DISCRETE:
            space, batch = spaces.Discrete(oc.DISCRETE[name]), oc.discrete_batch(oc.DISCRETE[name])
        else:
            space, batch = oc.make_box(spaces, name), oc.dtype_batch(name, target)
        t = _cuda(batch)
        if key in errors:
            if name in oc.DISCRETE:  # int64 -> uint8 keeps the low bits, in NumPy and here
                out = run_kernel(t, torch.empty(t.shape, dtype=torch.uint8, device="cuda"), _native.OBS_CAST)
                oc.assert_same_bits(_np(out), oc.cast(batch, np.uint8), key)
            continue
        w = oc.build(gw, stand_in(space, len(batch)), "dtype", target)
        oc.assert_same_bits(_np(w.observations(t)), gold[f"{key}/out"], key)
        oc.assert_same_bits(_np(t), batch, "the caller's tensor")
    if name == "wide64":
        x = oc.crafted(name)
        with np.errstate(all="ignore"):
            through = x.astype(np.float32).astype(np.float16)
        assert (oc.bits(gold["d/wide64/float16/out"]) != oc.bits(through))[~np.isnan(x)].any(), "the recording tells one rounding from two"


def test_rescale_of_the_float64_box(gold, errors):
    for target in ("same", "array"):
        x = oc.crafted("wide64")
        w = oc.build(gw, stand_in(oc.make_box(spaces, "wide64"), len(x)), "rescale", target, "wide64")
        t = _cuda(x)
        oc.assert_same_bits(_np(w.observations(t)), gold[f"r/wide64/{target}/out"], target)
        oc.assert_same_bits(_np(t), x, "the caller's tensor")


def test_a_view_that_starts_mid_allocation():
    """``traj["obs"][1:]`` of a 3-wide float32 trajectory of 5 sub-environments starts 60 bytes into the allocation, 12 bytes off a 16-byte boundary,
    while the result is aligned: no common head exists and the block goes element by element."""
    import torch

    name, T, N = "pendulum", 9, 5
    x = oc.tiled(oc.crafted(name), T * N).reshape(T, N, 3)
    traj = _cuda(x)
    view = traj[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 12
    w = oc.build(gw, stand_in(oc.make_box(spaces, name), N), "rescale", "pm1", name)
    got = w._observations_of_steps(view, T - 1)
    oc.assert_same_bits(_np(got), oc.affine(x[1:], w.gradient, w.intercept), "rescale of the view")
    w = oc.build(gw, stand_in(oc.make_box(spaces, name), N), "dtype", "float16")
    oc.assert_same_bits(_np(w._observations_of_steps(view, T - 1)), oc.cast(x[1:], np.float16), "float16 of the view")
    oc.assert_same_bits(_np(traj), x, "the caller's tensor")


@pytest.mark.parametrize("case", ["affine32", "affine64", "f64_f16", "f32_u8", "i64_f32"])
def test_kernel_on_views_at_every_offset(case):
    """Every pair of offsets of the input's and the output's first element within 16 bytes: the ones a common scalar head serves (vector body) and the ones
    it cannot (element by element), for counts below, at and above one group.  Nothing outside the output view is written."""
    import torch

    kind = _native.OBS_AFFINE if case.startswith("affine") else _native.OBS_CAST
    tin, tout, box = {"affine32": (torch.float32, torch.float32, "pendulum"), "affine64": (torch.float64, torch.float64, "level64"),
                      "f64_f16": (torch.float64, torch.float16, "level64"), "f32_u8": (torch.float32, torch.uint8, "level32"),
                      "i64_f32": (torch.int64, torch.float32, None)}[case]
    if box is None:
        src, dim = np.random.default_rng(5).integers(-2**40, 2**40, (70, 3)), 3
    else:
        src = oc.integer_batch(box, "uint8") if case == "f32_u8" else oc.crafted(box)
        dim = src.shape[1]
    rng = np.random.default_rng(6)
    g, c = rng.uniform(-2, 2, dim).astype(src.dtype), rng.uniform(-2, 2, dim).astype(src.dtype)
    np_out = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16, torch.uint8: np.uint8}[tout]
    for rows in (1, 2, 67):
        given = oc.tiled(src, rows)
        n = rows * dim
        want = oc.affine(given, g, c) if kind == _native.OBS_AFFINE else oc.cast(given, np_out)
        for in_off in range(4):
            for out_off in range(4):
                xbase = torch.zeros(n + 8, dtype=tin, device="cuda")
                obase = torch.full((n + 8,), 77, dtype=tout, device="cuda")
                xv, ov = xbase[in_off:in_off + n], obase[out_off:out_off + n]
                xv.copy_(_cuda(given).reshape(-1))
                if kind == _native.OBS_AFFINE:
                    run_kernel(xv, ov, kind, dim, _cuda(g), _cuda(c))
                else:
                    run_kernel(xv, ov, kind)
                got = _np(obase)
                assert (got[:out_off] == 77).all() and (got[out_off + n:] == 77).all(), (case, rows, in_off, out_off)
                oc.assert_same_bits(got[out_off:out_off + n].reshape(rows, dim), want, f"{case} rows={rows} offsets {in_off}/{out_off}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_kernel_with_humanoid_width(dtype):
    """obs_dim 348 (Humanoid-v5), 2 rows: more parameters than one sweep of the workgroup stages, and a row width that is no multiple of a group's."""
    import torch

    rng = np.random.default_rng(348)
    x, g, c = (rng.uniform(-3, 3, s).astype(dtype) for s in ((2, 348), 348, 348))
    out = run_kernel(_cuda(x), torch.empty((2, 348), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda"), _native.OBS_AFFINE, 348,
                     _cuda(g), _cuda(c))
    oc.assert_same_bits(_np(out), oc.affine(x, g, c))


def test_kernel_beyond_one_sweep_of_the_grid():
    """More groups than the grid has threads (2048 workgroups x 256 threads x 4 elements), with an odd row width: the parameter index of a thread's
    later groups moves by the stride's remainder."""
    import torch

    dim = 7
    rows = 2048 * 256 * 4 // dim + 12345
    rng = np.random.default_rng(9)
    x = rng.uniform(-3, 3, (rows, dim)).astype(np.float32)
    g, c = rng.uniform(-2, 2, dim).astype(np.float32), rng.uniform(-2, 2, dim).astype(np.float32)
    out = run_kernel(_cuda(x), torch.empty((rows, dim), dtype=torch.float32, device="cuda"), _native.OBS_AFFINE, dim, _cuda(g), _cuda(c))
    oc.assert_same_bits(_np(out), oc.affine(x, g, c))


def test_kernels_refuse_bad_arguments():
    import torch

    x = torch.zeros(66, device="cuda")
    g = torch.ones(2, device="cuda")
    with pytest.raises(_native.NativeError):  # obs_dim beyond what LDS is given
        run_kernel(x, torch.empty_like(x), _native.OBS_AFFINE, _native.OBS_MAX_DIM + 1, g, g)
    with pytest.raises(_native.NativeError):  # an affine map keeps its dtype
        run_kernel(x, torch.empty(66, dtype=torch.float64, device="cuda"), _native.OBS_AFFINE, 2, g, g)
    with pytest.raises(_native.NativeError):  # no parameters
        run_kernel(x, torch.empty_like(x), _native.OBS_AFFINE, 2)
    with pytest.raises(_native.NativeError):  # float16 is a target only
        run_kernel(x.to(torch.float16), torch.empty_like(x), _native.OBS_CAST)
    with pytest.raises(_native.NativeError):
        run_kernel(x, torch.empty_like(x), 2)
    s = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(_native.NativeError):
        run_one_hot([s] * 5, [2] * 5, torch.empty((4, 10), dtype=torch.int64, device="cuda"))
    with pytest.raises(_native.NativeError):
        run_one_hot([s], [0], torch.empty((4, 1), dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("rows", [1, 2, 65])
@pytest.mark.parametrize("name", ["frozenlake", "blackjack", "taxi"])
def test_one_hot_equals_the_reference_recording(gold, name, rows):
    """Widths 16, 45 (every other row starts 8 bytes off a 16-byte boundary) and 500; an output view 8 bytes off; a state outside its space."""
    import torch

    if name == "blackjack":
        space, parts, widths = oc.blackjack_space(spaces), tuple(oc.tiled(p, rows) for p in oc.blackjack_batch()), oc.BLACKJACK
    else:
        n = oc.DISCRETE[name]
        space, parts, widths = spaces.Discrete(n), (oc.tiled(oc.discrete_batch(n), rows),), (n,)
    want = oc.tiled(gold[f"f/{name}/out"], rows)
    w = gw.FlattenObservation(stand_in(space, rows))
    given = tuple(_cuda(p) for p in parts)
    got = w.observations(given if name == "blackjack" else given[0])
    oc.assert_same_bits(_np(got), want, f"{name} rows={rows}")
    for t, p in zip(given, parts):
        oc.assert_same_bits(_np(t), p, "the caller's tensor")
    if name == "blackjack":  # the [N, 3] block of a rollout, taken apart by its last axis
        oc.assert_same_bits(_np(w.observations(_cuda(np.stack(parts, axis=-1)))), want, "from the block")
    W = sum(widths)
    base = torch.full((rows * W + 3,), 77, dtype=torch.int64, device="cuda")
    view = base[1:1 + rows * W]
    assert view.data_ptr() % 16 == 8
    run_one_hot(given, widths, view)
    got = _np(base)
    assert got[0] == 77 and (got[1 + rows * W:] == 77).all()
    oc.assert_same_bits(got[1:1 + rows * W].reshape(rows, W), want, "into a view 8 bytes off")
    bad = [p.copy() for p in parts]
    bad[0][0], bad[-1][-1] = widths[0], -1  # one past the end; below the start
    out = run_one_hot([_cuda(p) for p in bad], widths, torch.empty((rows, W), dtype=torch.int64, device="cuda"))
    oc.assert_same_bits(_np(out), oc.one_hot(bad, widths), "states outside their space leave a zero segment")
    assert _np(out).sum() < rows * len(widths)


def test_flatten_of_a_box_is_a_view():
    x = _cuda(oc.crafted("pendulum").reshape(-1, 1, 3))
    w = gw.FlattenObservation(stand_in(spaces.Box(-1.0, 1.0, shape=(1, 3), dtype=np.float32), len(x)))
    got = w.observations(x)
    assert got.shape == (len(x), 3) and got.data_ptr() == x.data_ptr()


def test_a_target_the_device_does_not_cast_to_is_refused():
    w = gw.DtypeObservation(stand_in(oc.make_box(spaces, "level32"), 2), np.uint16)
    with pytest.raises(error.Error, match="float16, float32, float64, int32, int64, uint8"):
        w.observations(_cuda(np.ones((2, 5), np.float32)))


@pytest.mark.parametrize("key,mode", [(k, "NEXT_STEP") for k in oc.TRAJECTORIES] + [("cartpole_array", "DISABLED"), ("taxi_flat", "DISABLED"),
                                                                                   ("blackjack_flat", "DISABLED")])
def test_trajectories_with_device_tensors(gold, key, mode):
    env_id, kind, arg = oc.TRAJECTORIES[key]
    env = gymnasium_amd.make_vec(env_id, num_envs=oc.TRAJ_N, autoreset_mode=MODES[mode], output="torch")
    w = oc.build(gw, env, kind, arg, oc.BOX_OF_ENV.get(env_id))
    base = f"t/{key}/{mode}"
    obs, _ = w.reset(seed=oc.TRAJ_SEED)
    assert obs.is_cuda
    oc.assert_same_bits(_np(obs), gold[f"{base}/obs"][0], "reset")
    for t, a in enumerate(oc.trajectory_actions(env_id)):
        o, r, te, tr, _ = w.step(_cuda(a))
        assert o.is_cuda
        oc.assert_same_bits(_np(o), gold[f"{base}/obs"][t + 1], f"obs t={t}")
        assert np.array_equal(_np(r).astype(np.float64), gold[f"{base}/rewards"][t]), f"rewards t={t}"
        assert np.array_equal(_np(te), gold[f"{base}/flags"][0, t]) and np.array_equal(_np(tr), gold[f"{base}/flags"][1, t])
        if mode == "DISABLED":
            done = np.logical_or(_np(te), _np(tr))
            if done.any():
                o, _ = w.reset(options={"reset_mask": done})
            oc.assert_same_bits(_np(o), gold[f"{base}/post"][t], f"after the masked reset t={t}")
    w.close()


@pytest.mark.parametrize("env_id,kind,arg", [("CartPole-v1", "rescale", "array"), ("CartPole-v1", "dtype", "float64"), ("CartPole-v1", "flatten", None),
                                             ("Pendulum-v1", "rescale", "pm1"), ("Pendulum-v1", "dtype", "float16"), ("Pendulum-v1", "transform", None),
                                             ("Pendulum-v1", "reward", None), ("Taxi-v4", "flatten", None), ("Taxi-v4", "dtype", "float32"),
                                             ("Blackjack-v1", "flatten", None)])
def test_rollout_equals_steps(env_id, kind, arg):
    import torch

    T, N = 8, 64
    ea, eb = (gymnasium_amd.make_vec(env_id, num_envs=N, output="torch") for _ in range(2))
    a, b = (oc.build(gw, e, kind, arg, oc.BOX_OF_ENV.get(env_id)) for e in (ea, eb))
    a.reset(seed=9), b.reset(seed=9)
    b.action_space.seed(4)
    traj = b.rollout(T)
    steps = [a.step(traj["actions"][t]) for t in range(T)]
    for k, name in enumerate(("obs", "rewards", "terminations", "truncations")):
        want = torch.stack([s[k] for s in steps])
        if name == "obs":
            oc.assert_same_bits(_np(traj[name]), _np(want), f"{env_id} {kind} {name}")
        else:
            assert np.array_equal(_np(traj[name]), _np(want)), f"{env_id} {kind} {name}"
    full = b.rollout(2, traj["actions"][:2], infos=True, return_actions=False)  # the keywords pass through
    assert "infos" in full and "actions" not in full
    a.close(), b.close()


def test_stacking_with_the_statistics_wrappers():
    """Above a transform, NormalizeObservation runs its stand-alone pass over the transformed observations; below one, the fused unit keeps working."""
    import torch

    N, T = 64, 6
    envs = [gymnasium_amd.make_vec("Pendulum-v1", num_envs=N, output="torch") for _ in range(4)]
    # NormalizeObservation above RescaleObservation == above the same arithmetic written as two torch operations
    rescale = gw.RescaleObservation(envs[0], 0.0, 1.0)
    g, c = _cuda(rescale.gradient), _cuda(rescale.intercept)
    a = gw.NormalizeObservation(rescale)
    b = gw.NormalizeObservation(gw.TransformObservation(envs[1], lambda o: torch.mul(g, o).add(c)))
    assert not a._fused and not b._fused
    # DtypeObservation above a fused NormalizeObservation == the fused unit's output, cast
    inner = gw.NormalizeObservation(envs[2])
    top = gw.DtypeObservation(inner, np.float64)
    twin = gw.NormalizeObservation(envs[3])
    assert inner._fused and twin._fused and top.single_observation_space.dtype == np.float64
    assert not gw.NormalizeReward(top)._fused, "nothing above a transform joins the fused unit underneath"
    for w in (a, b, top, twin):
        w.reset(seed=2)
    acts = _cuda(oc.tiled(oc.trajectory_actions("Pendulum-v1").reshape(-1, 1), T * N).reshape(T, N, 1))
    for t in range(T):
        sa, sb, st, sw = (w.step(acts[t]) for w in (a, b, top, twin))
        oc.assert_same_bits(_np(sa[0]), _np(sb[0]), f"normalised rescaled observations t={t}")
        assert st[0].dtype == torch.float64
        oc.assert_same_bits(_np(st[0]), _np(sw[0]).astype(np.float64), f"cast normalised observations t={t}")
    assert np.array_equal(a.obs_rms.mean, b.obs_rms.mean) and np.array_equal(a.obs_rms.var, b.obs_rms.var)
    ra, rb = a.rollout(3, acts[:3]), b.rollout(3, acts[:3])
    oc.assert_same_bits(_np(ra["obs"]), _np(rb["obs"]), "rollout through both")
    rt, rw = top.rollout(3, acts[:3]), twin.rollout(3, acts[:3])
    oc.assert_same_bits(_np(rt["obs"]), _np(rw["obs"]).astype(np.float64), "rollout above the fused unit")
    for w in (a, b, top, twin):
        w.close()


def test_capture_is_refused():
    env = gymnasium_amd.make_vec("Pendulum-v1", num_envs=4, output="torch")
    env.reset(seed=0)
    for w in (gw.RescaleObservation(env, -1.0, 1.0), gw.DtypeObservation(env, np.float64), gw.FlattenObservation(env),
              gw.TransformObservation(env, oc.transform_func), gw.TransformReward(env, oc.reward_func)):
        with pytest.raises(error.Error, match="untransformed"):
            w.capture_steps(policy=lambda obs: obs[:, :1], steps=2)
    env.close()
