"""RepeatAction / StickyAction of the sub-environments for the MuJoCo ids, composed BY HAND over a plain env (helper of
test_mujoco_step_wrappers_host.py and test_gpu_mujoco_step_wrappers.py).

`Composition` runs the semantics of SyncVectorEnv over StickyAction(RepeatAction(TimeLimit(env), k), p, d) (gymnasium/wrappers/stateful_action.py:16-220,
vector/sync_vector_env.py:253-337) with nothing but the plain engine calls, on the oracle engine or the GPU engine: the plain env is made with
autoreset_mode="Disabled" and the helper applies the recorded mode's autoreset itself, with masked resets.  Per outer step:

  * the sticky decision of every row from a NumPy PCG64 placed at the row's words (get_rng_state()); the advanced words go back with the engine's
    seed-by-words call;
  * up to k plain steps; a row that is out of the series (finished inside the repeat, or in its autoreset step) is held still with get_state() /
    set_state() -- it is stepped with the others, with its flag cleared so that the DISABLED env does not refuse it, and then put back;
  * the record: observation, reward, flags, infos (assembled by the env's own _info_dict, as step() does), final rows, the inner step at which each row
    ended, the sticky decisions, the generator words, episode statistics and running totals as the vector level counts them (one step per step()).
"""
import numpy as np

NO_DRAW, DREW_NO, DREW_YES, IN_SERIES = 0, 1, 2, 3  # sticky decision of a row in one outer step
_M64 = (1 << 64) - 1


def uniform_at(words):
    """(np_random.uniform() of a Generator(PCG64) standing at `words` = {state_hi, state_lo, inc_hi, inc_lo}, the advanced state's two words)"""
    bg = np.random.PCG64()
    st = bg.state
    st["state"] = {"state": (int(words[0]) << 64) | int(words[1]), "inc": (int(words[2]) << 64) | int(words[3])}
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    u = np.random.Generator(bg).uniform()
    s = bg.state["state"]["state"]
    return u, s >> 64, s & _M64


class Composition:
    def __init__(self, env, k=0, p=0.0, d=0, mode="NextStep"):
        assert str(env.autoreset_mode).lower().endswith("disabled"), "the plain env is made with autoreset_mode='Disabled'"
        assert mode in ("NextStep", "SameStep", "Disabled")
        self.env, self.k, self.p, self.d, self.mode = env, int(k), float(p), int(d), mode
        self.N = env.num_envs
        self.totals = {"env_steps": 0, "reset_steps": 0, "episodes": 0, "length_sum": 0, "return_sum": 0.0}
        self._last_record = None
        self._clear(np.ones(self.N, dtype=bool), first=True)

    def _clear(self, rows, first=False):
        if first:
            self.has_last, self.taken = np.zeros(self.N, dtype=bool), np.zeros(self.N, dtype=np.int64)
            self.last = None
            self.pending = np.zeros(self.N, dtype=bool)
            self.ep_ret, self.ep_len = np.zeros(self.N), np.zeros(self.N, dtype=np.int64)
        cut = rows & (self.taken > 0)  # a series cut short by a reset
        self.has_last[rows], self.taken[rows], self.pending[rows] = False, 0, False
        self.ep_ret[rows], self.ep_len[rows] = 0.0, 0
        return cut

    def reset(self, seed=None):
        out = self.env.reset(seed=seed)
        self._clear(np.ones(self.N, dtype=bool))
        return out

    def reset_rows(self, mask):
        """a masked reset by the caller (DISABLED); returns (obs, infos, rows whose series it cut)"""
        mask = np.asarray(mask, dtype=bool)
        obs, infos = self.env.reset(options={"reset_mask": mask})
        cut = self._clear(mask)
        if self._last_record is not None:  # (the record of the step that finished these rows carries it, as under the other two modes)
            self._last_record["series_cut"] = self._last_record["series_cut"] | cut
        return np.array(obs), infos, cut

    def _fill_reset_info(self, rows, rinfos, mask):
        for name, start, width, in_reset in self.env._info_columns():
            if in_reset and name in rinfos:
                v = np.asarray(rinfos[name], dtype=np.float64)
                if width == 0:
                    rows[mask, start] = v[mask]
                else:
                    rows[mask, start:start + width] = v[mask]

    def step(self, actions):
        env, N, k = self.env, self.N, max(self.k, 1)
        a = np.array(actions, copy=True)
        if self.last is None:
            self.last = np.zeros_like(a)
        assert self.last.dtype == a.dtype, "the element type of the action rows must not change between steps"
        resetting = self.pending.copy() if self.mode == "NextStep" else np.zeros(N, dtype=bool)
        assert not (self.mode == "Disabled" and self.pending.any()), "DISABLED: reset the finished rows first (reset_rows)"
        stepping = ~resetting
        decisions = np.full(N, NO_DRAW, dtype=np.int8)
        cut = np.zeros(N, dtype=bool)
        if self.d:  # StickyAction.action of every row that steps; before anything else its generator does in this step
            words = env.get_rng_state().copy()
            moved = np.zeros(N, dtype=bool)
            for i in np.flatnonzero(stepping):
                stick = self.taken[i] > 0
                if stick:
                    decisions[i] = IN_SERIES
                elif self.has_last[i]:
                    u, hi, lo = uniform_at(words[i])
                    words[i, 0], words[i, 1], moved[i] = hi, lo, True
                    stick = u < self.p
                    decisions[i] = DREW_YES if stick else DREW_NO
                if stick:
                    a[i] = self.last[i]
                    self.taken[i] += 1
                if self.taken[i] == self.d:
                    self.taken[i] = 0
                self.last[i], self.has_last[i] = a[i], True
            if moved.any():
                env._engine.seed(words, moved.view(np.uint8))
        obs_dim = int(np.prod(env.single_observation_space.shape))
        obs = np.zeros((N, obs_dim))
        info_rows = None
        if resetting.any():  # the NEXT_STEP autoreset step: no draw, no repeat, reward 0, sticky state lost
            robs, rinfos = env.reset(options={"reset_mask": resetting})
            obs[resetting] = np.array(robs)[resetting]
            cut |= self._clear(resetting)
        total, single = np.zeros(N), np.zeros(N)
        te, tr = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
        inner_end = np.zeros(N, dtype=np.int64)
        active = stepping.copy()
        for j in range(k):
            if not active.any():
                break
            still = ~active
            if still.any():  # held still: stepped with its flag cleared, then put back
                st, el, fl = env.get_state()
                env.set_state(None, None, np.where(still, 0, fl).astype(np.uint8))
            o, r, t1, t2, _ = env.step(a)
            o, r, t1, t2 = np.array(o), np.array(r), np.array(t1, dtype=bool), np.array(t2, dtype=bool)
            inf = np.array(env._host(env._info)) if env._info is not None else np.zeros((N, 1))
            if still.any():
                st2, el2, fl2 = env.get_state()
                st2[still], el2[still], fl2[still] = st[still], el[still], fl[still]
                env.set_state(st2, el2, fl2)
            if info_rows is None:
                info_rows = np.zeros_like(inf)
            obs[active], info_rows[active] = o[active], inf[active]
            total[active] = total[active] + r[active]  # total_reward = 0.0; total_reward += float(reward)
            single[active] = r[active]
            te[active], tr[active] = t1[active], t2[active]
            inner_end[active] = j + 1
            active = active & ~(t1 | t2)
        reward = np.where(stepping, total if self.k > 0 else single, 0.0)
        done = te | tr
        self.ep_ret[stepping] += reward[stepping]
        self.ep_len[stepping] += 1
        rec = {"reward": reward, "terminated": te, "truncated": tr, "inner_end": inner_end, "decisions": decisions, "resetting": resetting,
               "ep_r": np.where(done, self.ep_ret, 0.0), "ep_l": np.where(done, self.ep_len, 0), "actions": a}
        t = self.totals
        t["env_steps"] += int(stepping.sum())
        t["reset_steps"] += int(resetting.sum())
        t["episodes"] += int(done.sum())
        t["length_sum"] += int(self.ep_len[done].sum())
        t["return_sum"] += float(self.ep_ret[done].sum())
        if info_rows is None:
            info_rows = np.zeros((N, max(int(env._engine.info_dim), 1)))  # (every row was in its autoreset step)
        final_obs, final_rows = obs.copy(), info_rows.copy()
        reset_rows = resetting.copy()
        if resetting.any():
            self._fill_reset_info(info_rows, rinfos, resetting)
        if self.mode == "SameStep" and done.any():  # final_obs / final_info: the last inner step's; the top-level entries: the reset's
            robs, rinfos2 = env.reset(options={"reset_mask": done})
            obs[done] = np.array(robs)[done]
            self._fill_reset_info(info_rows, rinfos2, done)
            cut |= self._clear(done)
            reset_rows |= done
        elif self.mode != "SameStep":
            self.pending = done.copy()
        infos = {}
        if env.INFO_KEYS:
            infos.update(env._info_dict(info_rows, np.ones(N, dtype=bool), reset_rows))
        if self.mode == "SameStep" and done.any():
            arr = np.full(N, None, dtype=object)
            for i in np.flatnonzero(done):
                arr[i] = final_obs[i].copy()
            infos["final_obs"], infos["_final_obs"] = arr, done.copy()
            infos["final_info"] = env._info_dict(final_rows, done, np.zeros(N, dtype=bool)) if env.INFO_KEYS else {}
            infos["_final_info"] = done.copy()
        rec.update(obs=obs.reshape((N,) + tuple(env.single_observation_space.shape)), infos=infos, final_obs=final_obs, final_info_rows=final_rows,
                   series_cut=cut, rng=env.get_rng_state().copy(), sticky_taken=self.taken.copy(), sticky_has_last=self.has_last.copy())
        self._last_record = rec
        return rec


def coverage(records, k, d):
    """What a run holds, from the records alone: a truncation / a termination at an inner step below k, sticky draws that triggered and that did
    not, series cut short by a reset."""
    inner = np.stack([r["inner_end"] for r in records])
    trunc = np.stack([r["truncated"] for r in records])
    term = np.stack([r["terminated"] for r in records])
    dec = np.stack([r["decisions"] for r in records])
    cut = np.stack([r["series_cut"] for r in records])
    return {"trunc_inside": int((trunc & ~term & (inner < k)).sum()) if k > 1 else 0, "term_inside_rows": int((term & (inner < k)).any(axis=0).sum()) if k > 1 else 0,
            "triggered": int((dec == DREW_YES).sum()), "not_triggered": int((dec == DREW_NO).sum()), "cut": int(cut.sum()) if d else 0}
