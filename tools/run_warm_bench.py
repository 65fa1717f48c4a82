#!/usr/bin/env python3
"""The telemetry-handler loop cold against warm-started ("the run() path"): mpc_run_batch_device and
mpc_run_batch_device_warm over --steps messages per car, the waypoint window (the rule of tests/run_warm_helpers.py) and the ideal
plant in torch on the device, and the latency of one message at B = 1 through mpc_run_batch_host(_warm) (what the drop-in's
MPC::run() calls).  One JSON line per measurement; needs an MI355X.  Every timed window ends in a device synchronise, every shape is
warmed up first, each figure is the median of --reps loops with their spread; the solve calls of a loop are timed with events of
their own.  The slowest solve of a step prices its launch: its iteration count is reported per step.

  python tools/run_warm_bench.py --mode cold      # works on a checkout without the warm entry points too (the parent's figures)
  python tools/run_warm_bench.py --mode warm [--out profiles/run_warm.json]   (--out appends the lines to the file's "rows")
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


def pick_window(torch, wp, x, y, npts=6):
    """tests/run_warm_helpers.py: pick_window, in torch: wp [n, 2] on the device -> ptsx, ptsy [npts, B]."""
    n = wp.shape[0]
    p = torch.stack([x, y], dim=1)
    j = torch.cdist(p, wp).argmin(dim=1)
    ahead = ((p - wp[j]) * (wp[(j + 1) % n] - wp[j])).sum(1) > 0
    k = torch.where(ahead, j, j - 1)
    idx = (k[None, :] + torch.arange(npts, device=wp.device)[:, None]) % n
    return wp[idx, 0].contiguous(), wp[idx, 1].contiguous()


def plant(torch, pose, out8, max_steering):
    c, s = torch.cos(pose[2]), torch.sin(pose[2])
    return torch.stack([pose[0] + out8[0] * c - out8[1] * s, pose[1] + out8[0] * s + out8[1] * c, pose[2] + out8[2], out8[3], out8[4] * max_steering,
                        out8[5]]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("cold", "warm"), required=True)
    ap.add_argument("--batches", default="65536,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--config", default="config-fast.json")
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, a.config))
    wp_host = np.asarray(pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv")), dtype=np.float64)
    warm = a.mode == "warm"
    base = {"tool": "tools/run_warm_bench.py", "tag": a.tag, "mode": a.mode, "config": a.config, "steps": a.steps}
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    wp = t(wp_host)
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r), flush=True)
    for B in [int(x) for x in a.batches.split(",") if x]:
        sc = pkg.scenarios.lake_track_batch(B, params, wp_host, seed=122)
        pose0 = t(sc["pose"])
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            wbuf = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=dev) if warm else None
            status = torch.empty((B,), dtype=torch.int32, device=dev)
            times = []; solve_ms = None; its = None; sts = None
            for rep in range(a.reps + 1):                     # the first loop warms up every shape
                pose = pose0.clone()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                it_steps = []; st_steps = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(a.steps):
                    px, py = pick_window(torch, wp, pose[0], pose[1])
                    ev[k][0].record()
                    if warm:
                        r = mpc.run_torch(pose, px, py, warm=wbuf if k else None, warm_status=status if k else None, warm_out=wbuf, status_out=status)
                    else:
                        r = mpc.run_torch(pose, px, py)
                    ev[k][1].record()
                    it_steps.append(r["iters"]); st_steps.append(r["status"].clone())
                    pose = plant(torch, pose, r["out8"], params.max_steering)
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t0)
                    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
                    solve_ms = ms if solve_ms is None else np.minimum(solve_ms, ms)
                its = torch.stack(it_steps).cpu().numpy(); sts = torch.stack(st_steps).cpu().numpy()
        med = float(np.median(times))
        emit(dict(base, B=B, kernel="lane" if B > 1024 else "wave", seconds_median=med, seconds_min=float(min(times)), seconds_max=float(max(times)),
                  reps=a.reps, solves_per_s=B * a.steps / med, what="whole loop: window, run(), plant",
                  run_call_ms_per_step_best=[round(float(x), 4) for x in solve_ms], run_call_ms_steps_2_on_median=float(np.median(solve_ms[1:])),
                  solves_per_s_run_calls_steps_2_on=B / (1e-3 * float(np.median(solve_ms[1:]))),
                  iters_per_solve_steps_2_on=float(its[1:].mean()), iters_per_solve_step_1=float(its[0].mean()),
                  slowest_solve_iterations_per_step=[int(x) for x in its.max(1)], non_success_solves=int((sts != 0).sum())))
    if not a.no_latency:
        # B = 1, host arrays in and out, one call per message as MPC::run() does it
        sc = pkg.scenarios.lake_track_batch(8, params, wp_host, seed=122)
        per = []; its = []
        with pkg.BatchedMPC(params, 1, device=0) as mpc:
            for car in range(8):
                for rep in range(2):                          # rep 0 warms up
                    pose = sc["pose"][:, car:car + 1].copy(); w = None; ws = None
                    for k in range(a.steps):
                        n = len(wp_host)
                        d = ((wp_host - pose[:2, 0]) ** 2).sum(1); j = int(d.argmin())
                        kk = j if ((pose[:2, 0] - wp_host[j]) * (wp_host[(j + 1) % n] - wp_host[j])).sum() > 0 else j - 1
                        idx = (kk + np.arange(6)) % n
                        px, py = wp_host[idx, 0][:, None].copy(), wp_host[idx, 1][:, None].copy()
                        t0 = time.perf_counter()
                        if warm:
                            r = mpc.run_numpy(pose, px, py, warm=w, warm_status=ws, want_warm=True)
                            w, ws = r["warm"], r["status"]
                        else:
                            r = mpc.run_numpy(pose, px, py)
                        dt_ = time.perf_counter() - t0
                        if rep and k:                         # messages 2..n: the ones a warm start changes
                            per.append(dt_); its.append(int(r["iters"][0]))
                        o = r["out8"][:, 0]; c, s = np.cos(pose[2, 0]), np.sin(pose[2, 0])
                        pose = np.array([[pose[0, 0] + o[0] * c - o[1] * s], [pose[1, 0] + o[0] * s + o[1] * c], [pose[2, 0] + o[2]], [o[3]],
                                         [o[4] * params.max_steering], [o[5]]])
        emit(dict(base, B=1, kernel="wave", what="one message through the host entry point, messages 2..n of 8 cars",
                  ms_median=1e3 * float(np.median(per)), ms_p10=1e3 * float(np.quantile(per, 0.1)), ms_p90=1e3 * float(np.quantile(per, 0.9)),
                  iters_per_solve=float(np.mean(its)), solves=len(per)))
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/run_warm_bench.py", "rows": []}
        doc["rows"] += lines
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
