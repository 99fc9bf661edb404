"""mi_discretize_observations / mi_discretize_actions against the torch composition a user would write without them, in one process on one GPU.

    python scripts/discretize_bench.py [--rows 8388608] [--iters 50] [--out result.json]

Observations: 65 536 x 128 Pendulum rows, bins = (10, 10, 10), flat form, against one torch.bucketize per dimension plus the multiply-adds.  Actions:
the same number of flat indices at Ant's 8 dimensions (bins = 3: every index takes the 32-bit path; bins = 17: prod(bins) > 2^31, the 64-bit path)
against torch's floor remainder / division and a gather per dimension.  Both sides are timed with device events over ``iters`` launches after a warm-up,
alternating, three rounds; the best round of each is reported with the fraction of the 8 TB/s HBM roofline on ALGORITHMIC bytes (observations: 12 B in
+ 8 B out per row; actions: 8 B in + 32 B out per row).  The outputs of the two sides are compared first."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12


def timed(fn, iters, torch):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def compare(name, ours, theirs, bytes_per_call, iters, torch):
    for _ in range(3):
        ours(), theirs()
    torch.cuda.synchronize()
    best = {"kernel": float("inf"), "torch": float("inf")}
    for _ in range(3):
        best["kernel"] = min(best["kernel"], timed(ours, iters, torch))
        best["torch"] = min(best["torch"], timed(theirs, iters, torch))
    return {"case": name, "kernel_us": best["kernel"] * 1e6, "torch_us": best["torch"] * 1e6, "speedup": best["torch"] / best["kernel"],
            "algorithmic_bytes": bytes_per_call, "kernel_fraction_of_8TBps": bytes_per_call / best["kernel"] / HBM_BYTES_PER_S,
            "torch_fraction_of_8TBps": bytes_per_call / best["torch"] / HBM_BYTES_PER_S}


def main():
    import torch

    from gymnasium_amd import _native

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536 * 128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _native.load_library()
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows, results = args.rows, []
    gen = torch.Generator(device=dev).manual_seed(1)

    # observations: Pendulum, bins = (10, 10, 10)
    low, high = np.array([-1, -1, -8], np.float32), np.array([1, 1, 8], np.float32)
    bins = np.array([10, 10, 10], np.int32)
    edges = [np.linspace(low[i], high[i], bins[i] + 1)[1:-1] for i in range(3)]
    hi_clip = high - 1e-8
    params = torch.from_numpy(np.concatenate([low, hi_clip] + edges).astype(np.float32)).to(dev)
    x = (torch.rand((rows, 3), generator=gen, device=dev) * 2.2 - 1.1) * torch.tensor([1.0, 1.0, 8.0], device=dev)
    out = torch.empty(rows, dtype=torch.int64, device=dev)
    t_edges, t_lo, t_hi = [torch.from_numpy(e).to(dev) for e in edges], torch.from_numpy(low).to(dev), torch.from_numpy(hi_clip).to(dev)

    def ours_obs():
        lib.check(lib.discretize_observations(0, stream, C.c_void_p(x.data_ptr()), _native.MI_F32, rows, 3, bins.ctypes.data, C.c_void_p(params.data_ptr()),
                                              C.c_void_p(params.data_ptr() + 12), C.c_void_p(params.data_ptr() + 24), 0, C.c_void_p(out.data_ptr())))
        return out

    def torch_obs():
        clipped = torch.minimum(torch.maximum(x, t_lo), t_hi)
        idx = torch.bucketize(clipped[:, 0], t_edges[0], right=True)
        for d in (1, 2):
            idx = idx * int(bins[d]) + torch.bucketize(clipped[:, d], t_edges[d], right=True)
        return idx

    assert torch.equal(ours_obs(), torch_obs()), "the two sides disagree on the observations"
    results.append(compare("observations pendulum bins=(10,10,10)", ours_obs, torch_obs, rows * (12 + 8), args.iters, torch))

    # actions: Ant's 8 dimensions
    for b in (3, 17):
        abins = np.full(8, b, np.int32)
        centers = 0.5 * (np.linspace(np.float32(-1), np.float32(1), b + 1)[:-1] + np.linspace(np.float32(-1), np.float32(1), b + 1)[1:])
        table = torch.from_numpy(np.tile(centers.astype(np.float32), 8)).to(dev)
        t_centers = torch.from_numpy(centers.astype(np.float32)).to(dev)
        idx = torch.randint(0, b ** 8, (rows,), generator=gen, device=dev, dtype=torch.int64)
        act = torch.empty((rows, 8), dtype=torch.float32, device=dev)

        def ours_act():
            lib.check(lib.discretize_actions(0, stream, C.c_void_p(idx.data_ptr()), _native.MI_I64, rows, 8, abins.ctypes.data, C.c_void_p(table.data_ptr()), 0,
                                             C.c_void_p(act.data_ptr()), _native.MI_F32))
            return act

        def torch_act():
            f, cols = idx, []
            for _ in range(8):
                cols.insert(0, t_centers[torch.remainder(f, b)])
                f = torch.div(f, b, rounding_mode="floor")
            return torch.stack(cols, dim=1)

        assert torch.equal(ours_act(), torch_act()), "the two sides disagree on the actions"
        results.append(compare(f"actions ant bins={b} ({'32' if b ** 8 < 2 ** 31 else '64'}-bit path)", ours_act, torch_act, rows * (8 + 32), args.iters, torch))

    for r in results:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": rows, "iters": args.iters, "device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
