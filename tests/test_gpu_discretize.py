"""GPU side of wrappers.DiscretizeObservation / DiscretizeAction (csrc/discretize.hip): direct kernel calls bit for bit against what was recorded from
the reference (tests/golden/discretize.npz; rows are independent, so a recording tiles to any size), and the wrappers end to end against the recorded
SyncVectorEnv trajectories in the three autoreset modes.  No input is chosen to fault a kernel: out-of-range indices are defined behaviour (they wrap
or clamp)."""
import ctypes as C

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import AutoresetMode, error

import discretize_cases as dc

pytestmark = pytest.mark.gpu

FIX = dc.fixture()
MODES = {"next": AutoresetMode.NEXT_STEP, "same": AutoresetMode.SAME_STEP, "disabled": AutoresetMode.DISABLED}
ROWS = (1, 63, 64, 65, 257)
CODES = {np.dtype(np.float32): _native.MI_F32, np.dtype(np.float64): _native.MI_F64, np.dtype(np.int64): _native.MI_I64, np.dtype(np.int32): _native.MI_I32}


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what):
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True), what


def stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# -- 1. the kernels, called directly ------------------------------------------------------------------------------------------------------------------
def call_observations(case, x, bins=None, shift=0):
    """mi_discretize_observations over ``x`` ([rows, D] host array) with the recorded tables of ``case``; ``shift``: input and output start that many
    elements into their buffers (a view that is not 16-byte aligned)."""
    import torch

    name, case_bins, multi = dc.OBS_CASES[case]
    low, _ = dc.box_arrays(name)
    b = np.ascontiguousarray(dc.bins_array(name, case_bins) if bins is None else bins, dtype=np.int32)
    lo, hi, edges = cuda(low), cuda(FIX[f"o/{case}/hi_clip"]), cuda(FIX[f"o/{case}/edges"].astype(low.dtype))
    xt = torch.zeros(x.size + shift, dtype=getattr(torch, x.dtype.name), device="cuda")[shift:].view(x.shape)
    xt.copy_(cuda(x))
    shape = (len(x), len(low)) if multi else (len(x),)
    out = torch.full((int(np.prod(shape)) + shift,), -7, dtype=torch.int64, device="cuda")[shift:].view(shape)
    assert xt.data_ptr() % 16 == (shift * x.itemsize) % 16
    lib = _native.load_library()
    lib.check(lib.discretize_observations(0, stream(), C.c_void_p(xt.data_ptr()), CODES[x.dtype], len(x), len(low), b.ctypes.data, C.c_void_p(lo.data_ptr()),
                                          C.c_void_p(hi.data_ptr()), C.c_void_p(edges.data_ptr()) if edges.numel() else None, int(multi),
                                          C.c_void_p(out.data_ptr())))
    return out


def call_actions(case, x, centers=None, bins=None):
    import torch

    name, case_bins, multi = dc.ACT_CASES[case]
    low, _ = dc.box_arrays(name)
    b = np.ascontiguousarray(dc.bins_array(name, case_bins) if bins is None else bins, dtype=np.int32)
    table = cuda((FIX[f"a/{case}/centers"] if centers is None else centers).astype(low.dtype))
    xt = cuda(x)
    out = torch.full((len(x), len(low)), -7.0, dtype=getattr(torch, low.dtype.name), device="cuda")
    lib = _native.load_library()
    lib.check(lib.discretize_actions(0, stream(), C.c_void_p(xt.data_ptr()), CODES[x.dtype], len(x), len(low), b.ctypes.data, C.c_void_p(table.data_ptr()),
                                     int(multi), C.c_void_p(out.data_ptr()), CODES[low.dtype]))
    return out


@pytest.mark.parametrize("case", list(dc.OBS_CASES))
def test_observation_kernel_equals_the_recording(case):
    x, y = FIX[f"o/{case}/x"], FIX[f"o/{case}/y"]
    same(call_observations(case, x), y, "the recording as it is")
    for rows in ROWS:
        same(call_observations(case, dc.tiled(x[::-1], rows)), dc.tiled(y[::-1], rows), rows)
    same(call_observations(case, dc.tiled(x, 300), shift=1), dc.tiled(y, 300), "a view off the 16-byte boundary")


@pytest.mark.parametrize("case", list(dc.ACT_CASES))
def test_action_kernel_equals_the_recording(case):
    x, y = FIX[f"a/{case}/x"], FIX[f"a/{case}/y"]
    same(call_actions(case, x), y, "the recording as it is")
    for rows in ROWS:
        same(call_actions(case, dc.tiled(x[::-1], rows)), dc.tiled(y[::-1], rows), rows)
    narrow = (np.abs(x) < 2 ** 31) if x.ndim == 1 else (np.abs(x) < 2 ** 31).all(axis=1)
    same(call_actions(case, x[narrow].astype(np.int32)), y[narrow], "int32 indices")


def test_both_division_paths_are_in_the_recording():
    x = FIX["a/ant_3/x"]
    assert ((x >= 0) & (x < 2 ** 31)).sum() > 200 and (x >= 2 ** 31).any() and (x < -2 ** 31).any() and (x == -1).any()  # both paths in one launch
    assert int(FIX["a/ant_3/single"][0]) < 2 ** 31 < int(FIX["a/ant_17/single"][0]) and int(FIX["a/humanoid_4/single"][0]) == 2 ** 34


def test_the_table_cap():
    """A table AT the cap runs (observations: the recorded one_cap; actions: MAX_TABLE centres against the NumPy path); one entry more is refused by the
    entry points, as the constructors refuse it."""
    same(call_observations("one_cap", FIX["o/one_cap/x"][:300]), FIX["o/one_cap/y"][:300], "at the cap")
    with pytest.raises(_native.NativeError):
        call_observations("one_cap", FIX["o/one_cap/x"][:4], bins=[dc.MAX_TABLE + 2])
    centers = np.linspace(-2, 2, dc.MAX_TABLE, dtype=np.float32)
    x = np.array([0, 1, dc.MAX_TABLE - 1, dc.MAX_TABLE, -1, 2 ** 40 + 1], dtype=np.int64)
    same(call_actions("one_7", x, centers=centers, bins=[dc.MAX_TABLE]), centers[x % dc.MAX_TABLE][:, None], "at the cap")
    with pytest.raises(_native.NativeError):
        call_actions("one_7", x, centers=np.zeros(dc.MAX_TABLE + 1, np.float32), bins=[dc.MAX_TABLE + 1])


@pytest.mark.parametrize("T", [1, 5])
def test_block_form_is_one_launch_over_all_rows(T):
    """``rollout``'s [T, N, ...] blocks through the wrappers' device paths, at an N that is no multiple of the tile."""
    act_wrapper, obs_wrapper = dc.act_wrapper, dc.obs_wrapper
    n = 67
    for case in ("pendulum_345", "acrobot_mixed_multi", "wide64_345"):
        x, y = FIX[f"o/{case}/x"], FIX[f"o/{case}/y"]
        w = obs_wrapper(case, rows=n)
        same(w._apply(cuda(dc.tiled(x, T * n).reshape((T, n) + x.shape[1:])), 2), dc.tiled(y, T * n).reshape((T, n) + y.shape[1:]), (case, T))
    for case in ("ant_3", "ant_17", "humanoid_mixed_multi", "act64_345"):
        x, y = FIX[f"a/{case}/x"], FIX[f"a/{case}/y"]
        w = act_wrapper(case, rows=n)
        same(w._actions_of_steps(cuda(dc.tiled(x, T * n).reshape((T, n) + x.shape[1:])), T), dc.tiled(y, T * n).reshape((T, n) + y.shape[1:]), (case, T))
    with pytest.raises(TypeError):
        act_wrapper("one_7", rows=3).actions(cuda(np.zeros(3, np.float32)))


# -- 2. end to end ------------------------------------------------------------------------------------------------------------------------------------
def make(name, mode, n, output, **kw):
    kw.setdefault("max_episode_steps", dc.LIMIT)
    return gymnasium_amd.make_vec(dc.TRAJ[name][0], num_envs=n, output=output, autoreset_mode=MODES[mode], **kw)


def give(a, output):
    return cuda(a) if output == "torch" else a.copy()


def final_rows(infos, like):
    """(rows, mask) of a step's final_obs: an int64 tensor beside its mask, or the NumPy infos' object array."""
    fo, fm = np.zeros_like(like), np.zeros(len(like), dtype=bool)
    if "final_obs" in infos:
        fm = host(infos["_final_obs"]).astype(bool)
        final = infos["final_obs"]
        if hasattr(final, "cpu"):
            assert final.dtype == cuda(like).dtype
            fo[fm] = host(final)[fm]
        else:
            for i in np.flatnonzero(fm):
                assert isinstance(final[i], int) == (like.ndim == 1)
                fo[i] = final[i]
    return fo, fm


def run_against_recording(name, mode, n, output):
    """reset, T steps and the masked resets; the first N rows are the recording's (sub-environment i is seeded with SEED + i whatever the batch size)."""
    k = f"t/{name}/{mode}"
    w = dc.wrap(wrappers, make(name, mode, n, output), name)
    obs0, _ = w.reset(seed=dc.SEED)
    same(host(obs0)[:dc.N], FIX[f"{k}/obs0"], "obs0")
    assert (output == "torch") == hasattr(obs0, "is_cuda")
    for t in range(dc.T):
        o, r, te, tr, infos = w.step(give(dc.tiled(FIX[f"{k}/actions"][t], n), output))
        same(host(o)[:dc.N], FIX[f"{k}/obs"][t], ("obs", t)), same(host(r)[:dc.N], FIX[f"{k}/rewards"][t], ("rewards", t))
        same(host(te)[:dc.N], FIX[f"{k}/term"][t], ("term", t)), same(host(tr)[:dc.N], FIX[f"{k}/trunc"][t], ("trunc", t))
        if mode == "same":
            fo, fm = final_rows(infos, host(o))
            same(fm[:dc.N], FIX[f"{k}/final_mask"][t], ("final mask", t)), same(fo[:dc.N], FIX[f"{k}/final_obs"][t], ("final_obs", t))
        mask = (host(te) | host(tr)) if mode == "disabled" else np.zeros(n, dtype=bool)
        if t == dc.MASK_AT:
            mask = mask | dc.tiled(dc.MASK, n)
        same(mask[:dc.N], FIX[f"{k}/reset_mask"][t], ("reset mask", t))
        if mask.any():
            ro, _ = w.reset(options={"reset_mask": mask.copy()})
            same(host(ro)[:dc.N], FIX[f"{k}/reset_obs"][t], ("masked reset", t))
    w.close()


@pytest.mark.parametrize("name,mode", dc.TRAJ_KEYS)
def test_trajectories_equal_the_recordings_device_tensors(name, mode):
    run_against_recording(name, mode, dc.N, "torch")


@pytest.mark.parametrize("name,mode,n,output", [("pendulum_flat", "same", 3, "numpy"), ("pendulum_multi", "same", 67, "numpy"), ("acrobot_flat", "next", 67, "numpy"),
                                                ("mountaincar_onehot", "disabled", 3, "numpy"), ("mountaincar_continuous_multi", "disabled", 67, "numpy"),
                                                ("pendulum_flat", "next", 67, "torch"), ("pendulum_multi", "same", 67, "torch"),
                                                ("mountaincar_onehot", "next", 67, "torch"), ("mountaincar_continuous_multi", "disabled", 67, "torch")])
def test_trajectories_equal_the_recordings_other_sizes_and_numpy(name, mode, n, output):
    run_against_recording(name, mode, n, output)


def first_reset(k):
    """The number of recorded steps before the first masked reset."""
    return int(np.flatnonzero(FIX[f"{k}/reset_mask"].any(axis=1))[0]) + 1


@pytest.mark.parametrize("with_infos", [False, True])
@pytest.mark.parametrize("name,mode", dc.TRAJ_KEYS)
def test_rollout_equals_the_recording(name, mode, with_infos):
    k, n = f"t/{name}/{mode}", 67
    steps = first_reset(k)
    w = dc.wrap(wrappers, make(name, mode, n, "torch"), name)
    w.reset(seed=dc.SEED)
    block = cuda(np.stack([dc.tiled(a, n) for a in FIX[f"{k}/actions"][:steps]]))
    if mode == "disabled" and with_infos:  # the engine has no rollout launch under DISABLED: the steps are collected, and their infos are refused
        with pytest.raises(error.Error):
            w.rollout(steps, block, infos=True)
        w.close()
        return
    out = w.rollout(steps, block, **({"infos": True} if with_infos else {}))
    same(host(out["obs"])[:, :dc.N], FIX[f"{k}/obs"][:steps], "obs"), same(host(out["rewards"])[:, :dc.N], FIX[f"{k}/rewards"][:steps], "rewards")
    same(host(out["terminations"])[:, :dc.N], FIX[f"{k}/term"][:steps], "term"), same(host(out["truncations"])[:, :dc.N], FIX[f"{k}/trunc"][:steps], "trunc")
    assert ("infos" in out) == with_infos
    if with_infos and mode == "same":
        fm = FIX[f"{k}/final_mask"][:steps]
        same(host(out["infos"]["_final_obs"])[:, :dc.N], fm, "final mask")
        got = host(out["infos"]["final_obs"])[:, :dc.N]
        assert got.dtype == np.int64 and np.array_equal(got[fm], FIX[f"{k}/final_obs"][:steps][fm])
    w.close()


@pytest.mark.parametrize("mode", ["next", "same"])
@pytest.mark.parametrize("name", ["pendulum_flat", "mountaincar_continuous_multi"])
def test_rollout_equals_steps_through_the_wrappers(name, mode):
    """rollout(8) == 8 x step(): with given index blocks, and with the wrapper's own host draws (the same seeded space on both sides)."""
    import torch

    T, n = 8, 67
    a, b = (dc.wrap(wrappers, make(name, mode, n, "torch"), name) for _ in range(2))
    a.reset(seed=3), b.reset(seed=3)
    a.action_space.seed(9), b.action_space.seed(9)
    acts = torch.stack([cuda(np.asarray(a.action_space.sample()) - 2) for _ in range(T)])  # (indices below zero among them)
    [b.action_space.sample() for _ in range(T)]
    for given in (acts, None):
        traj = a.rollout(T, given)
        steps = [b.step(acts[t] if given is not None else b.action_space.sample()) for t in range(T)]
        for key, pos in (("obs", 0), ("rewards", 1), ("terminations", 2), ("truncations", 3)):
            same(traj[key], host(torch.stack([s[pos] for s in steps])), (key, given is None))
    a.close(), b.close()


def test_captured_steps_through_discretize_action_equal_the_eager_loop():
    import torch

    def policy(obs):  # indices from -24 to 24 over 7 bins: they wrap
        return (obs[:, 2] * 3.0).to(torch.int64)

    n, K = 64, 4
    a, b = (wrappers.DiscretizeAction(gymnasium_amd.make_vec("Pendulum-v1", num_envs=n, output="torch"), 7) for _ in range(2))
    oa, _ = a.reset(seed=3)
    ob, _ = b.reset(seed=3)
    oa, ob = a.step(policy(oa))[0], b.step(policy(ob))[0]  # one eager step before a capture (HipVectorEnv.capture_steps)
    graphed = b.capture_steps(policy=policy, steps=K)
    for _ in range(2):
        for _ in range(K):
            oa, ra, tea, tra, _ = a.step(policy(oa))
        got = graphed.replay()
        for x, y in zip((oa, ra, tea, tra), got[:4]):
            assert np.array_equal(host(x), host(y))
    buf = torch.zeros((n,), dtype=torch.int64, device="cuda")
    graphed = b.capture_steps(actions=buf, steps=1)
    for v in (5, -3):
        buf.fill_(v)
        want, got = a.step(buf.clone()), graphed.replay()
        for k in range(4):
            assert np.array_equal(host(want[k]), host(got[k])), (v, k)
    with pytest.raises(error.Error):
        b.capture_steps(policy="random", steps=2)
    with pytest.raises(error.Error):
        wrappers.DiscretizeObservation(b, 4).capture_steps(steps=1)
    a.close(), b.close()


def test_one_hot_tile_coding_over_the_flat_form():
    """FlattenObservation(DiscretizeObservation(env)): the recorded one-hot rows, and every row has exactly one 1 at the flat index."""
    w = dc.wrap(wrappers, make("mountaincar_onehot", "next", 67, "torch"), "mountaincar_onehot")
    obs, _ = w.reset(seed=dc.SEED)
    same(host(obs)[:dc.N], FIX["t/mountaincar_onehot/next/obs0"], "the recorded rows")
    assert host(obs).shape == (67, 16) and np.array_equal(host(obs).sum(axis=1), np.ones(67, dtype=np.int64))
    v = wrappers.DiscretizeObservation(make("mountaincar_onehot", "next", 67, "torch"), 4)
    assert np.array_equal(host(obs).argmax(axis=1), host(v.reset(seed=dc.SEED)[0]))
    v.close()
    w.close()
