#!/usr/bin/env python3
"""Closed loops cold against warm-started: solves/s and iterations per solve of mpc_rollout_batch_device and
mpc_rollout_batch_device_warm, and the latency of one closed-loop solve at B = 1 through the host entry points (what the drop-in's
MPC::solve() calls).  One JSON line per measurement; needs an MI355X.  Every timed window ends in a device synchronise, every
shape is warmed up first, and each figure is the median of --reps windows with their spread.

  python tools/warm_rollout_bench.py --mode cold      # works on a checkout without the warm entry points too (the parent's figures)
  python tools/warm_rollout_bench.py --mode warm [--shift 1]
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
    ap.add_argument("--mode", choices=("cold", "warm"), required=True)
    ap.add_argument("--batches", default="65536,1024")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--config", default="config-fast.json")
    ap.add_argument("--shift", type=int, default=-1, help="MpcWarmOpts.shift (-1: the library's default)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-latency", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, a.config))
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    warm = a.mode == "warm"
    opts = None
    if warm:
        opts = pkg.warm_opts_default() if a.shift < 0 else pkg.warm_opts_default(shift=a.shift)
    base = {"tool": "tools/warm_rollout_bench.py", "tag": a.tag, "mode": a.mode, "config": a.config, "steps": a.steps,
            "opts": None if not warm else {"shift": opts.shift, "mu_init": opts.mu_init, "bound_push": opts.bound_push, "duals": opts.duals}}
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    for B in [int(x) for x in a.batches.split(",") if x]:
        sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=122)
        state0, coeffs, ylo, yhi = t(sc["state"]), t(sc["coeffs"]), t(sc["yaw_lo"]), t(sc["yaw_hi"])
        kw = dict(warm_start=True, warm_opts=opts) if warm else {}
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            times = []
            for rep in range(a.reps + 1):                     # the first window warms up every shape
                state = state0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ro = mpc.rollout_torch(state, coeffs, ylo, yhi, steps=a.steps, want_hist=False, **kw)
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t0)
            status = ro["status"].cpu().numpy(); iters = ro["iters"].cpu().numpy()
        ok = status == 0
        r = dict(base, B=B, kernel="lane" if B > 1024 else "wave", seconds_median=float(np.median(times)), seconds_min=float(min(times)),
                 seconds_max=float(max(times)), reps=a.reps, solves_per_s=B * a.steps / float(np.median(times)),
                 iters_per_solve=float(iters.sum()) / (B * a.steps), iters_per_solve_converged_cars=float(iters[ok].mean()) / a.steps,
                 cars_all_steps_success=int(ok.sum()))
        print(json.dumps(r), flush=True)
    if not a.no_latency:
        # B = 1, host arrays in and out, one call per step as MPC::solve() does it (src/test.cpp:79-111)
        sc = pkg.scenarios.lake_track_batch(8, params, wp, seed=122)
        with pkg.BatchedMPC(params, 1, device=0) as mpc:
            per = []; its = []
            for car in range(8):
                for rep in range(2):                          # rep 0 warms up
                    st = sc["state"][:, car:car + 1].copy(); w = None; ws = None
                    args = (sc["coeffs"][:, car:car + 1], sc["yaw_lo"][car:car + 1], sc["yaw_hi"][car:car + 1])
                    for k in range(a.steps):
                        t0 = time.perf_counter()
                        if warm:
                            r = mpc.solve_numpy_warm(st, *args, warm=w, warm_status=ws, warm_opts=opts)
                            w, ws = r["warm"], r["status"]
                        else:
                            r = mpc.solve_numpy(st, *args)
                        dt_ = time.perf_counter() - t0
                        if rep and k:                         # steps 2..n: the ones a warm start changes
                            per.append(dt_); its.append(int(r["iters"][0]))
                        st = r["out"][:6].copy()
        print(json.dumps(dict(base, B=1, kernel="wave", what="one closed-loop solve through the host entry point, steps 2..n of 8 cars",
                              ms_median=1e3 * float(np.median(per)), ms_p10=1e3 * float(np.quantile(per, 0.1)), ms_p90=1e3 * float(np.quantile(per, 0.9)),
                              iters_per_solve=float(np.mean(its)), solves=len(per))), flush=True)


if __name__ == "__main__":
    main()
