"""-m gpu: ClipAction / RescaleAction / TransformAction with device tensors (mi_transform_actions, gymnasium_amd/csrc/action_wrappers.hip).

The kernel is compared bit for bit (integer views, NaN by position) with what the REFERENCE's wrappers forwarded
(tests/golden/action_wrappers.npz; rows are transformed independently, so a recording tiles to any batch size) and, where no recording exists,
with the NumPy restatement of tests/action_wrapper_cases.py, which tests/test_action_wrappers.py pins on the same recording.
"""
import ctypes as C

import numpy as np
import pytest

import action_wrapper_cases as ac
import gymnasium_amd
from conftest import golden
from gymnasium_amd import _native
from gymnasium_amd import wrappers as gw
from gymnasium_amd.gym_api import batch_space, error, spaces

pytestmark = pytest.mark.gpu
BY_DIM = {1: "pendulum", 7: "pusher", 8: "ant", 17: "humanoid"}


@pytest.fixture(scope="module")
def gold():
    return golden("action_wrappers.npz")


@pytest.fixture(scope="module")
def errors(gold):
    return dict(str(e).split("=") for e in gold["errors"])


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _parameters(gold, name, tr):
    """(kind, p0, p1) of mi_transform_actions for the recorded stack ``tr`` over box ``name``."""
    dim, bound = ac.BOXES[name]
    if tr == "clip":
        return _native.TRANSFORM_CLIP, np.full(dim, -bound, np.float32), np.full(dim, bound, np.float32)
    if tr == "clip01":
        return _native.TRANSFORM_CLIP, np.zeros(dim, np.float32), np.ones(dim, np.float32)
    gradient, intercept = gold[f"a/{name}/{tr}/params"]
    return _native.TRANSFORM_AFFINE_INVERSE, intercept, gradient


def run_kernel(x, out, kind, p0, p1, dim):
    """mi_transform_actions on torch's current stream; ``x`` / ``out``: device tensors (views allowed) of the same number of elements."""
    import torch

    lib = _native.load_library()
    code = {torch.float32: _native.MI_F32, torch.float64: _native.MI_F64}
    q0, q1 = np.ascontiguousarray(p0, np.float64), np.ascontiguousarray(p1, np.float64)
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel()
    lib.check(lib.transform_actions(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(x.data_ptr()), code[x.dtype],
                                    C.c_void_p(out.data_ptr()), code[out.dtype], x.numel(), dim, kind, q0.ctypes.data, q1.ctypes.data))
    return out


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("N", [1, 3, 67, 130])
@pytest.mark.parametrize("dim", list(BY_DIM))
def test_kernel_equals_the_reference_recording(gold, dim, N, T):
    import torch

    name = BY_DIM[dim]
    x = ac.inputs(name)
    for tr in ac.TRANSFORMS:
        kind, p0, p1 = _parameters(gold, name, tr)
        for inp in ("f32", "f64"):
            want = ac.tiled(gold[f"a/{name}/{tr}/{inp}"], T * N).reshape(T, N, dim)
            block = _cuda(ac.tiled(x[inp], T * N).reshape(T, N, dim))
            out = torch.empty(block.shape, dtype=torch.float64 if want.dtype == np.float64 else torch.float32, device="cuda")
            run_kernel(block, out, kind, p0, p1, dim)
            ac.assert_same_bits(_np(out), want, f"{name} {tr} {inp} N={N} T={T}")
            ac.assert_same_bits(_np(block), ac.tiled(x[inp], T * N).reshape(T, N, dim), "the input block")


@pytest.mark.parametrize("in_dtype,out_dtype", [("f32", "f32"), ("f64", "f32"), ("f64", "f64")])
def test_kernel_on_views_that_start_off_a_16_byte_boundary(gold, in_dtype, out_dtype):
    """Every pair of offsets of the input's and the output's first element within 16 bytes: the ones a common scalar head serves (vector body)
    and the ones it cannot (element by element), for counts below, at and above one group.  Nothing outside the output view is written."""
    import torch

    name, dim = "pusher", 7
    tdt = {"f32": torch.float32, "f64": torch.float64}
    src = ac.inputs(name)[in_dtype]
    for tr in ("clip", "rescale01"):
        kind, p0, p1 = _parameters(gold, name, tr)
        for rows in (1, 2, 67):
            n = rows * dim
            given = ac.tiled(src, rows)
            formula = ac.clip if kind == _native.TRANSFORM_CLIP else ac.affine_inverse
            want = formula(given, p0, p1, np.float64 if out_dtype == "f64" else np.float32)
            for in_off in range(4):
                for out_off in range(4):
                    xbase = torch.zeros(n + 8, dtype=tdt[in_dtype], device="cuda")
                    obase = torch.full((n + 8,), -77.0, dtype=tdt[out_dtype], device="cuda")
                    xv, ov = xbase[in_off:in_off + n], obase[out_off:out_off + n]
                    xv.copy_(_cuda(given).reshape(-1))
                    run_kernel(xv, ov, kind, p0, p1, dim)
                    got = _np(obase)
                    assert (got[:out_off] == -77.0).all() and (got[out_off + n:] == -77.0).all(), (tr, rows, in_off, out_off)
                    ac.assert_same_bits(got[out_off:out_off + n].reshape(rows, dim), want, f"{tr} rows={rows} offsets {in_off}/{out_off}")


@pytest.mark.parametrize("inp", ["f32", "f64"])
def test_kernel_beyond_one_sweep_of_the_grid(inp):
    """More groups than the grid has threads (2048 workgroups x 256 threads x 4 elements), with an odd row width: the parameter index of a thread's
    later groups moves by the stride's remainder."""
    import torch

    name, dim = "pusher", 7
    rows = 2048 * 256 * 4 // dim + 12345
    given = ac.tiled(ac.inputs(name)[inp], rows)
    low, high = np.full(dim, -2.0, np.float32) * np.arange(1, dim + 1, dtype=np.float32) / dim, np.full(dim, 2.0, np.float32)
    g, i = ac.rescale_parameters(low, high, 0.0, 1.0)
    x = _cuda(given)
    for kind, p0, p1, want in ((_native.TRANSFORM_CLIP, low, high, ac.clip(given, low, high)),
                               (_native.TRANSFORM_AFFINE_INVERSE, i, g, ac.affine_inverse(given, i, g))):
        out = run_kernel(x, torch.empty(x.shape, dtype=torch.float32, device="cuda"), kind, p0, p1, dim)
        ac.assert_same_bits(_np(out), want, f"kind {kind}")


def test_kernel_refuses_bad_arguments():
    import torch

    x = torch.zeros(66, device="cuda")
    for dim in (0, 33):
        with pytest.raises(_native.NativeError):
            run_kernel(x, torch.empty_like(x), _native.TRANSFORM_CLIP, np.zeros(max(dim, 1)), np.ones(max(dim, 1)), dim)
    with pytest.raises(_native.NativeError):  # float32 in, float64 out: no row of the reference comes out wider than it went in
        run_kernel(x, torch.empty(66, dtype=torch.float64, device="cuda"), _native.TRANSFORM_CLIP, np.zeros(2), np.ones(2), 2)
    with pytest.raises(_native.NativeError):
        run_kernel(x, torch.empty_like(x), 2, np.zeros(2), np.ones(2), 2)


@pytest.mark.parametrize("name", list(ac.BOXES))
def test_wrappers_with_device_tensors_equal_the_reference_recording(gold, errors, name):
    """``actions()`` of every recorded stack for float32, float64 and int64 tensors, a non-contiguous tensor and a view that starts mid-row."""
    import torch

    x = ac.inputs(name)
    rows, dim = x["f64"].shape
    for tr in ac.TRANSFORMS:
        w = ac.build(gw, ac.SpacesOnlyEnv(spaces, batch_space, ac.make_box(spaces, name), rows), tr)
        for inp in ("f32", "f64", "i64"):
            key = f"a/{name}/{tr}/{inp}"
            given = _cuda(x[inp])
            if key in errors:
                with pytest.raises(TypeError):
                    w.actions(given)
                continue
            got = w.actions(given)
            assert got.is_cuda and got.data_ptr() != given.data_ptr()
            ac.assert_same_bits(_np(got), gold[key], key)
            ac.assert_same_bits(_np(given), x[inp], "the caller's tensor")
            if inp == "i64":
                continue
            transposed = _cuda(x[inp].T.copy()).t()  # (rows, dim) with strides (1, rows)
            assert dim == 1 or not transposed.is_contiguous()
            ac.assert_same_bits(_np(w.actions(transposed)), gold[key], key + " non-contiguous")
            flat = torch.zeros(rows * dim + 1, dtype=given.dtype, device="cuda")
            flat[1:].copy_(given.reshape(-1))
            view = flat[1:].reshape(rows, dim)
            assert view.is_contiguous() and view.data_ptr() % 16 != 0
            ac.assert_same_bits(_np(w.actions(view)), gold[key], key + " unaligned view")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("tr", ac.TRAJ_WRAPPERS)
@pytest.mark.parametrize("env_name", list(ac.TRAJ_ENVS))
def test_trajectories_with_device_tensors(gold, env_name, tr, dtype):
    key = f"b/{env_name}/{tr}/{np.dtype(dtype).name}"
    env = gymnasium_amd.make_vec(ac.TRAJ_ENVS[env_name], num_envs=ac.TRAJ_N, output="torch")
    w = ac.build(gw, env, tr)
    obs, _ = w.reset(seed=ac.TRAJ_SEED)
    assert np.array_equal(_np(obs), gold[f"{key}/obs"][0])
    for t, a in enumerate(_cuda(ac.trajectory_actions(env_name, dtype))):
        o, r, te, tr_, _ = w.step(a)
        assert o.is_cuda and np.array_equal(_np(o), gold[f"{key}/obs"][t + 1]), f"obs t={t}"
        assert np.array_equal(_np(r), gold[f"{key}/rewards"][t]), f"rewards t={t}"
        assert np.array_equal(_np(te), gold[f"{key}/flags"][0, t]) and np.array_equal(_np(tr_), gold[f"{key}/flags"][1, t])
    w.close()


def _restated(tr, env, a):
    """What the stack ``tr`` over ``env`` forwards for the array ``a``, from the restatement."""
    box = env.single_action_space
    if tr == "clip":
        return ac.clip(a, box.low, box.high)
    g, i = ac.rescale_parameters(box.low, box.high, 0.0, 1.0)
    if tr == "rescale01":
        return ac.affine_inverse(a, i, g)
    return ac.affine_inverse(ac.clip(a, np.zeros_like(box.low), np.ones_like(box.high)), i, g)  # clip01


def _twin_actions(rng, env, steps, dtype):
    box = env.single_action_space
    a = rng.uniform(-1.5, 1.5, (steps, env.num_envs) + box.shape) * box.high
    a[rng.random(a.shape) < 0.1] = 0.0
    return a.astype(dtype)


@pytest.mark.parametrize("tr", ["clip", "rescale01", "clip01"])
@pytest.mark.parametrize("env_id", ["HalfCheetah-v5", "Ant-v5", "Humanoid-v5"])
def test_mujoco_twins(env_id, tr):
    """``w.step(a)`` on one env == ``step(restated(a))`` on its twin, bit for bit, float32 and float64 batches in turn."""
    ea, eb = (gymnasium_amd.make_vec(env_id, num_envs=4, output="torch") for _ in range(2))
    w = ac.build(gw, ea, tr)
    oa, _ = w.reset(seed=5)
    ob, _ = eb.reset(seed=5)
    assert np.array_equal(_np(oa), _np(ob))
    rng = np.random.default_rng(2)
    for t in range(8):
        a = _twin_actions(rng, eb, 1, np.float32 if t % 2 == 0 else np.float64)[0]
        got, want = w.step(_cuda(a)), eb.step(_cuda(_restated(tr, eb, a)))
        for k in range(4):
            assert got[k].dtype == want[k].dtype and np.array_equal(_np(got[k]), _np(want[k])), (env_id, tr, t, k)
    w.close(), eb.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("env_id,tr", [("Pendulum-v1", "clip"), ("MountainCarContinuous-v0", "clip_rescale_pm1"), ("Ant-v5", "rescale01"),
                                       ("Pendulum-v1", "rescale_same")])
def test_rollout_with_actions_equals_steps(env_id, tr, dtype):
    import torch

    T, N = 5, 67
    ea, eb = (gymnasium_amd.make_vec(env_id, num_envs=N, output="torch") for _ in range(2))
    a, b = ac.build(gw, ea, tr), ac.build(gw, eb, tr)
    a.reset(seed=9), b.reset(seed=9)
    given = _twin_actions(np.random.default_rng(4), ea, T, dtype)
    acts = _cuda(given)
    steps = [a.step(acts[t]) for t in range(T)]
    traj = b.rollout(T, acts)
    for k, name in enumerate(("obs", "rewards", "terminations", "truncations")):
        assert np.array_equal(_np(torch.stack([s[k] for s in steps])), _np(traj[name])), (env_id, tr, name)
    ac.assert_same_bits(_np(traj["actions"]), given, "traj['actions'] holds the actions as the wrapper received them")
    ac.assert_same_bits(_np(acts), given, "the caller's block")
    full = b.rollout(T, acts, infos=True, return_actions=False)  # the keywords pass through
    assert "infos" in full and "actions" not in full
    a.close(), b.close()


def test_rollout_under_the_normalising_wrappers():
    """NormalizeReward(NormalizeObservation(ClipAction(env))): bit-equal to the same stack WITHOUT ClipAction fed the restated actions (the same
    passes on the same numbers), statistics included; and equal to five ``step()`` calls through the stack within what
    tests/test_gpu_wrapped_rollout.py grants the step and the whole-trajectory passes of the two normalisations against each other (batch
    moments summed in another order: observations rtol 2e-5 / atol 2e-6, rewards rtol 2e-6, statistics rtol 1e-5); flags exact."""
    import torch

    T, N = 5, 67
    envs = [gymnasium_amd.make_vec("Pendulum-v1", num_envs=N, output="torch") for _ in range(3)]
    stack = lambda e: gw.NormalizeReward(gw.NormalizeObservation(e))  # noqa: E731
    a, b, c = stack(gw.ClipAction(envs[0])), stack(gw.ClipAction(envs[1])), stack(envs[2])
    assert b.env._fused and b._fused, "the fused unit extends across the action wrapper"
    for w in (a, b, c):
        w.reset(seed=9)
    given = _twin_actions(np.random.default_rng(6), envs[0], T, np.float32)
    traj = b.rollout(T, _cuda(given))
    twin = c.rollout(T, _cuda(ac.clip(given, envs[2].single_action_space.low, envs[2].single_action_space.high)))
    for k in ("obs", "rewards", "terminations", "truncations"):
        assert np.array_equal(_np(traj[k]), _np(twin[k])), k
    ac.assert_same_bits(_np(traj["actions"]), given)
    assert np.array_equal(b.env.obs_rms.mean, c.env.obs_rms.mean) and np.array_equal(b.env.obs_rms.var, c.env.obs_rms.var)
    assert np.array_equal(b.return_rms.var, c.return_rms.var) and np.array_equal(b.accumulated_reward, c.accumulated_reward)
    steps = [a.step(_cuda(given[t])) for t in range(T)]
    np.testing.assert_allclose(_np(torch.stack([s[0] for s in steps])), _np(traj["obs"]), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(_np(torch.stack([s[1] for s in steps])), _np(traj["rewards"]), rtol=2e-6, atol=1e-12)
    assert np.array_equal(_np(torch.stack([s[2] for s in steps])), _np(traj["terminations"]))
    assert np.array_equal(_np(torch.stack([s[3] for s in steps])), _np(traj["truncations"]))
    np.testing.assert_allclose(a.env.obs_rms.mean, b.env.obs_rms.mean, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(a.env.obs_rms.var, b.env.obs_rms.var, rtol=1e-5, atol=1e-9)
    assert a.env.obs_rms.count == b.env.obs_rms.count and a.return_rms.count == b.return_rms.count
    assert np.array_equal(a.accumulated_reward, b.accumulated_reward)
    np.testing.assert_allclose(a.return_rms.var, b.return_rms.var, rtol=1e-9)
    for w in (a, b, c):
        w.close()


@pytest.mark.parametrize("env_id,tr", [("Pendulum-v1", "clip"), ("Ant-v5", "rescale01"), ("MountainCarContinuous-v0", "clip_rescale_pm1")])
def test_rollout_without_actions_equals_the_sample_loop(env_id, tr):
    import torch

    T, N = 5, 3
    ea, eb = (gymnasium_amd.make_vec(env_id, num_envs=N, output="torch") for _ in range(2))
    a, b = ac.build(gw, ea, tr), ac.build(gw, eb, tr)
    a.reset(seed=2), b.reset(seed=2)
    a.action_space.seed(ac.SAMPLE_SEED), b.action_space.seed(ac.SAMPLE_SEED)
    drawn, steps = [], []
    for _ in range(T):
        drawn.append(a.action_space.sample())
        steps.append(a.step(drawn[-1]))
    traj = b.rollout(T)
    ac.assert_same_bits(_np(traj["actions"]), np.stack(drawn), "the drawn actions, untransformed")
    for k, name in enumerate(("obs", "rewards", "terminations", "truncations")):
        assert np.array_equal(_np(torch.stack([s[k] for s in steps])), _np(traj[name])), name
    ac.assert_same_bits(a.action_space.sample(), b.action_space.sample(), "both spaces moved on by T draws")
    a.close(), b.close()


def _policy(obs):
    return 3.0 * obs[:, :1] - 0.5  # leaves Pendulum's +-2 and the wrapper's +-1 for part of the batch


@pytest.mark.parametrize("tr", ["clip", "clip_rescale_pm1"])
def test_captured_steps_equal_the_eager_loop(tr):
    N, K = 64, 4
    ea, eb = (gymnasium_amd.make_vec("Pendulum-v1", num_envs=N, output="torch") for _ in range(2))
    a, b = ac.build(gw, ea, tr), ac.build(gw, eb, tr)
    oa, _ = a.reset(seed=3)
    ob, _ = b.reset(seed=3)
    oa, ob = a.step(_policy(oa))[0], b.step(_policy(ob))[0]  # one eager step before a capture (HipVectorEnv.capture_steps)
    graphed = b.capture_steps(policy=_policy, steps=K)
    for _ in range(2):
        for _ in range(K):
            oa, ra, tea, tra, _ = a.step(_policy(oa))
        got = graphed.replay()
        for x, y in zip((oa, ra, tea, tra), got[:4]):
            assert np.array_equal(_np(x), _np(y))
    # ... and with an action tensor the captured steps read at replay time
    import torch

    buf = torch.zeros((N, 1), dtype=torch.float32, device="cuda")
    graphed = b.capture_steps(actions=buf, steps=1)
    for v in (5.0, -0.25):
        buf.fill_(v)
        want, got = a.step(buf.clone()), graphed.replay()
        for k in range(4):
            assert np.array_equal(_np(want[k]), _np(got[k])), (v, k)
    a.close(), b.close()


def test_random_policy_is_refused():
    env = gymnasium_amd.make_vec("Pendulum-v1", num_envs=4, output="torch")
    env.reset(seed=0)
    for w in (gw.ClipAction(env), gw.RescaleAction(env, -1.0, 1.0), gw.TransformAction(env, lambda a: a)):
        with pytest.raises(error.Error):
            w.capture_steps(policy="random", steps=2)
    env.close()


def test_transform_action_with_device_tensors():
    import torch

    T, N = 5, 4
    ea, eb = (gymnasium_amd.make_vec("Pendulum-v1", num_envs=N, output="torch") for _ in range(2))
    w = gw.TransformAction(ea, lambda a: a * 0.5)
    w.reset(seed=1), eb.reset(seed=1)
    acts = _cuda(_twin_actions(np.random.default_rng(1), ea, T, np.float32))
    traj = w.rollout(T, acts)
    steps = [eb.step(acts[t] * 0.5) for t in range(T)]
    assert np.array_equal(_np(traj["obs"]), _np(torch.stack([s[0] for s in steps]))) and np.array_equal(_np(traj["actions"]), _np(acts))
    got, want = w.step(acts[0]), eb.step(acts[0] * 0.5)
    assert np.array_equal(_np(got[0]), _np(want[0])) and np.array_equal(_np(got[1]), _np(want[1]))
    w.close(), eb.close()
