"""Time the observation-transform passes of gymnasium_amd.wrappers against the torch expression a user would otherwise write, A and B interleaved in
one process (device events around each call; the median of the repeats):

    python scripts/observation_wrappers_bench.py [--repeats 30] [--out FILE.json]

  rescale   RescaleObservation over a [128, 65536, 4] float32 trajectory            vs  g * x + c
  dtype     DtypeObservation float64 -> float32 over a [128, 65536, 4] trajectory   vs  x.to(torch.float32)
  one_hot   FlattenObservation of Taxi-v4's Discrete(500) over [2, 65536] states    vs  torch.nn.functional.one_hot(x, 500)

Bytes are what the pass must move (input read once, output written once); the fraction is of the 8.0 TB/s HBM3E peak.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

HBM_PEAK = 8.0e12


def main():
    import torch

    import observation_wrapper_cases as oc
    from gymnasium_amd import wrappers as gw
    from gymnasium_amd.gym_api import AutoresetMode, batch_space, spaces

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    T, N = 128, 65536
    gen = torch.Generator(device="cuda").manual_seed(0)

    def stand_in(space):
        return oc.SpacesOnlyEnv(spaces, batch_space, space, N, AutoresetMode.NEXT_STEP)

    cases = {}
    box = spaces.Box(np.array([-4.8, -3.0, -0.42, -3.5], np.float32), np.array([4.8, 3.0, 0.42, 3.5], np.float32), dtype=np.float32)
    w = gw.RescaleObservation(stand_in(box), -1.0, 1.0)
    x = torch.rand((T, N, 4), device="cuda", generator=gen) * 6 - 3
    g, c = torch.from_numpy(w.gradient).cuda(), torch.from_numpy(w.intercept).cuda()
    cases["rescale"] = (lambda: w._observations_of_steps(x, T), lambda: g * x + c, x.numel() * 8)
    x64 = torch.rand((T, N, 4), device="cuda", generator=gen, dtype=torch.float64)
    wd = gw.DtypeObservation(stand_in(spaces.Box(-1.0, 1.0, shape=(4,), dtype=np.float64)), np.float32)
    cases["dtype"] = (lambda: wd._observations_of_steps(x64, T), lambda: x64.to(torch.float32), x64.numel() * 12)
    rows = (2, N)
    states = torch.randint(0, 500, rows, device="cuda", generator=gen)
    wf = gw.FlattenObservation(stand_in(spaces.Discrete(500)))
    cases["one_hot"] = (lambda: wf._observations_of_steps(states, 2), lambda: torch.nn.functional.one_hot(states, 500), states.numel() * (8 + 500 * 8))
    result = {"shape": [T, N, 4], "one_hot_rows": rows[0] * rows[1], "repeats": args.repeats}
    for name, (ours, theirs, nbytes) in cases.items():
        a, b = ours(), theirs()
        same = bool(torch.equal(a, b))
        del a, b
        times = {"ours": [], "torch": []}
        for _ in range(3):  # warm-up of both
            ours(), theirs()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for label, fn in (("ours", ours), ("torch", theirs)):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                out = fn()
                end.record()
                end.synchronize()
                del out
                times[label].append(start.elapsed_time(end) * 1e-3)
        med = {k: statistics.median(v) for k, v in times.items()}
        result[name] = {"bytes": nbytes, "equal_to_torch": same,
                        **{f"{k}_ms": round(v * 1e3, 4) for k, v in med.items()},
                        **{f"{k}_min_ms": round(min(times[k]) * 1e3, 4) for k in times},
                        **{f"{k}_GBps": round(nbytes / v / 1e9, 1) for k, v in med.items()},
                        **{f"{k}_hbm_fraction": round(nbytes / v / HBM_PEAK, 3) for k, v in med.items()}}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
