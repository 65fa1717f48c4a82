#!/usr/bin/env python3
"""The closed-loop rollout stepwise against fused: mpc_rollout_batch_device(_warm), a launch per step, and
mpc_rollout_batch_device_fused, one launch in which every car advances on its own -- the same handle, the same build, the two
forms ALTERNATING loop by loop.  Each figure is the median of --reps loops after one warm-up loop of either form, a host clock
around a stream synchronise.  Reported with the times: iterations per solve and the per-car totals (max and mean over the cars),
the quantities the iteration-count bound of section 6j is stated in, and whether the two forms wrote the same bits.  Needs an
MI355X.

  python tools/rollout_fused_bench.py [--out profiles/rollout_fused.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,8192")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--config", default="config-fast.json")
    ap.add_argument("--seed", type=int, default=122)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_fused.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, a.config))
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    rows = []
    for B in [int(x) for x in a.batches.split(",") if x]:
        sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=a.seed)
        state0, coeffs, ylo, yhi = t(sc["state"]), t(sc["coeffs"]), t(sc["yaw_lo"]), t(sc["yaw_hi"])
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            for warm in (False, True):
                times = {False: [], True: []}; last = {}
                for rep in range(a.reps + 1):                 # the first loop of either form warms up
                    for fused in (False, True):
                        state = state0.clone()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        r = mpc.rollout_torch(state, coeffs, ylo, yhi, steps=a.steps, warm_start=warm, fused=fused)
                        torch.cuda.synchronize()
                        if rep:
                            times[fused].append(time.perf_counter() - t0)
                        last[fused] = (r, state)
                info = mpc.rollout_fused_info()
                same = all(torch.equal(last[False][0][k], last[True][0][k]) for k in ("status", "iters")) and torch.equal(last[False][1], last[True][1]) and \
                    bool(((last[False][0]["hist"] == last[True][0]["hist"]) | (last[False][0]["hist"].isnan() & last[True][0]["hist"].isnan())).all())
                it = last[True][0]["iters"].cpu().numpy().astype(np.int64); st = last[True][0]["status"].cpu().numpy()
                row = {"tool": "tools/rollout_fused_bench.py", "config": a.config, "seed": a.seed, "B": B, "steps": a.steps, "warm_start": warm, "reps": a.reps,
                       "fused_equals_stepwise_bitwise": same, "fused_kernel_ran": info["fused_launches"] > 0,
                       "iters_per_solve": float(it.mean() / a.steps), "car_total_iters_max": int(it.max()), "car_total_iters_mean": float(it.mean()),
                       "cars_with_a_solve_that_did_not_succeed": int((st != 0).sum())}
                for fused, name in ((False, "stepwise"), (True, "fused")):
                    med = float(np.median(times[fused]))
                    row[name] = {"seconds_median": med, "seconds_min": float(min(times[fused])), "seconds_max": float(max(times[fused])),
                                 "solves_per_s": B * a.steps / med}
                row["time_fused_over_stepwise"] = row["fused"]["seconds_median"] / row["stepwise"]["seconds_median"]
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"tool": "tools/rollout_fused_bench.py", "rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
