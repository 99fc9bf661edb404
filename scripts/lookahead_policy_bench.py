#!/usr/bin/env python3
"""lookahead_policy() against the only way to score K closed-loop policies before it, one MI355X, one session.

    python scripts/lookahead_policy_bench.py [--rounds 3] [--parent PATH/TO/PARENT/libmi355env.so] [--out profiles/lookahead_policy_ab.txt]

Every round is a process of its own, this build's and -- with --parent -- the parent build's interleaved (scripts/bench_rounds.py).  A process measures, for CartPole-v1 and Pendulum-v1, hidden = 0 and 64,
H = 128, gamma = 0.99 and K x N = 64 x 1024 (65 536 lanes) and 256 x 1024 (262 144 lanes), the time per scored batch -- device events around CALLS
calls, the variants of a configuration taken in turn window by window, median window -- of

  policy         env.lookahead_policy(params[K, P], 128, hidden=h): one launch, the path the host chooses (LDS at these shapes)
  policy_global  the same call with MI355ENV_LOOKAHEAD_POLICY_PATH=global
  eager          a second env of K * N sub-environments, H x (batched torch linear [+ relu + linear], argmax for the Discrete id, step())
  graph          the same H steps captured once with capture_steps(policy=..., steps=H) and replayed

and, for the two parameter paths alone, K x N = 4096 x 16 (a wavefront's lanes read four rows).  The baselines are given what favours them: the
set_state() that would put the K * N sub-environments into the tiled present state before every batch is NOT timed, nor is any reduction of their
rewards to returns; they run on from wherever the last batch left them (autoreset), which costs a step the same.  N(0, 1) weights.  Experiment
infrastructure only: no test reads its numbers.
"""
import argparse
import json
import os
import sys

from bench_rounds import finish, median_window, run_rounds, spread

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, WINDOWS, WARMUP = 128, 5, 3
CALLS = {"policy": 40, "policy_global": 40, "eager": 8, "graph": 8}
IDS = {"CartPole-v1": (4, 2), "Pendulum-v1": (3, 1)}  # obs_dim, outputs
SHAPES = ((64, 1024, True), (256, 1024, True), (4096, 16, False))  # K, N, with the baselines
PATH_VAR = "MI355ENV_LOOKAHEAD_POLICY_PATH"


def child():
    sys.path.insert(0, ROOT)
    import torch

    import gymnasium_amd

    def timed(call, n):
        return median_window(torch, call, 0, n, 1)  # us per call, one window

    def torch_policy(env_id, params, hidden, K, N):
        obs_dim, A = IDS[env_id]
        if hidden == 0:
            W, b = params[:, :A * obs_dim].reshape(K, A, obs_dim).transpose(1, 2).contiguous(), params[:, A * obs_dim:].reshape(K, 1, A)
            net = lambda x: torch.baddbmm(b, x, W)
        else:
            at = [hidden * obs_dim, hidden * obs_dim + hidden, hidden * obs_dim + hidden + A * hidden]
            W1, b1 = params[:, :at[0]].reshape(K, hidden, obs_dim).transpose(1, 2).contiguous(), params[:, at[0]:at[1]].reshape(K, 1, hidden)
            W2, b2 = params[:, at[1]:at[2]].reshape(K, A, hidden).transpose(1, 2).contiguous(), params[:, at[2]:].reshape(K, 1, A)
            net = lambda x: torch.baddbmm(b2, torch.relu(torch.baddbmm(b1, x, W1)), W2)
        if A > 1:
            return lambda obs: net(obs.view(K, N, obs_dim)).argmax(-1).reshape(K * N)
        return lambda obs: net(obs.view(K, N, obs_dim)).reshape(K * N, 1)

    out = {}
    for env_id, (obs_dim, A) in IDS.items():
        for hidden in (0, 64):
            for K, N, baselines in SHAPES:
                P = A * (obs_dim + 1) if hidden == 0 else hidden * (obs_dim + 1) + A * (hidden + 1)
                params = torch.randn((K, P), generator=torch.Generator().manual_seed(3)).cuda()
                env = gymnasium_amd.make_vec(env_id, num_envs=N, output="torch", copy=False)
                env.reset(seed=0)

                def policy_call(path):
                    def call():
                        if path:
                            os.environ[PATH_VAR] = path
                        else:
                            os.environ.pop(PATH_VAR, None)
                        env.lookahead_policy(params, H, 0.99, hidden=hidden)
                    return call

                variants = {"policy": policy_call(None), "policy_global": policy_call("global")}
                big = None
                if baselines:
                    big = gymnasium_amd.make_vec(env_id, num_envs=K * N, output="torch", copy=False)
                    big.reset(seed=0)
                    pol = torch_policy(env_id, params, hidden, K, N)

                    def eager():
                        obs = big._obs
                        for _ in range(H):
                            obs = big.step(pol(obs))[0]

                    big.step(pol(big._obs))  # (kernels load on first use, which a capture must not trigger)
                    graph = big.capture_steps(policy=pol, steps=H)
                    variants["eager"], variants["graph"] = eager, graph.replay
                for name, call in variants.items():
                    for _ in range(WARMUP):
                        call()
                torch.cuda.synchronize()
                took = {name: [] for name in variants}
                for _ in range(WINDOWS):
                    for name, call in variants.items():
                        took[name].append(timed(call, CALLS[name]))
                os.environ.pop(PATH_VAR, None)
                out[f"{env_id} h={hidden} K={K} N={N}"] = {name: sorted(v)[len(v) // 2] for name, v in took.items()}
                env.close()
                if big is not None:
                    big.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    rows, lines = run_rounds(__file__, args.rounds, args.parent, timeout=900)
    lines.append("")
    lines.append(f"us per scored batch (K candidates x N sub-environments x {H} steps); median [min .. max] of {args.rounds} processes; x = against `policy`")
    for (cfg, name, what), v in sorted(rows.items()):
        base = sorted(rows[(cfg, name, "policy")])
        lines.append(f"{cfg:34s} {name:6s} {what:14s} {spread(v, 10)}  x{sorted(v)[len(v) // 2] / base[len(base) // 2]:.2f}")
    finish(lines, args.out)


if __name__ == "__main__":
    main()
