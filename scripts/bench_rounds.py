"""The per-process round scheme of scripts/lookahead_bench.py and scripts/lookahead_policy_bench.py: every measurement runs in a process of its own
(`script --child`, which prints one `RESULT {configuration: {what: us}}` line), `rounds` times, this build's and -- with `parent`, the path of another
build's libmi355env.so -- the parent build's interleaved, the order alternating from round to round (MI355ENV_LIBRARY selects the build).  Experiment
infrastructure only."""
import json
import os
import subprocess
import sys


def run_rounds(script, rounds, parent=None, timeout=900):
    """-> ({(configuration, build, what): [us of every round]}, the raw lines, one per process)"""
    builds = [("this", None)] + ([("parent", parent)] if parent else [])
    rows, lines = {}, []
    for r in range(rounds):
        for name, lib in (builds if r % 2 == 0 else builds[::-1]):
            env = dict(os.environ)
            if lib:
                env["MI355ENV_LIBRARY"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(script), "--child"], env=env, capture_output=True, text=True, timeout=timeout)
            hit = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not hit:
                raise SystemExit(f"{name} child failed ({p.returncode}): {p.stdout[-400:]} {p.stderr[-1600:]}")
            res = json.loads(hit[-1][7:])
            for cfg, row in res.items():
                for what, us in row.items():
                    rows.setdefault((cfg, name, what), []).append(us)
            lines.append(f"round {r} {name}: " + json.dumps(res))
            print(lines[-1], flush=True)
    return rows, lines


def median_window(torch, call, warmup, calls, windows):
    """us per call: `warmup` calls, then device events around `calls` calls, `windows` times; the median window"""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    took = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            call()
        t1.record()
        torch.cuda.synchronize()
        took.append(t0.elapsed_time(t1) / calls * 1e3)
    return sorted(took)[len(took) // 2]


def spread(v, width):
    """'median [min .. max]' of one row, every figure `width` wide"""
    v = sorted(v)
    return f"{v[len(v) // 2]:{width}.1f} [{v[0]:{width}.1f} .. {v[-1]:{width}.1f}]"


def finish(lines, out_path):
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
