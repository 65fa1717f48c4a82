#!/usr/bin/env python3
"""What to hand a warm-started run() from the previous run() ("the run() path"): the decision on record.
CPU only, on the CPU build tests/run_warm_twin; two populations of telemetry-handler loops (window rule and ideal plant of
tests/run_warm_helpers.py), every solve against the oracle's cold mpc_run of the same instance.

Rows: the previous vehicle-frame record as it is / with psi projected into the new psi box (what the library does) / rigidly
re-framed into the new vehicle frame and projected (done here in numpy on the buffer between calls, not in the library), each with
MpcWarmOpts.shift 0 / 1 and mu_init 1e-6 / 1e-4.  Rule (section 6i's own): the fewest total iterations over both populations among the
rows without a status difference.   python tools/run_warm_grid.py [--out profiles/run_warm_grid.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G   # noqa: E402
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ   # noqa: E402
from run_warm_helpers import closed_loop, load_run_warm_twin, oracle_runs, run_differences, twin_run, twin_solve_box   # noqa: E402

POPULATIONS = (("config-fast.json", 96, 20), ("config-stable.json", 64, 12))


def run_post(params, pre, r9):
    """MPC.cpp:360-381 in numpy (csrc/mpc_run_core.h: run_post), for the "as it is" rows, whose solve does not go through run()."""
    myc, target, v0 = pre[13], pre[14], pre[3]
    steer = r9[6] + np.where(np.abs(myc) > params.steer_adj_thresh, params.steer_adj_ratio * myc, 0.0)
    sv = np.clip(steer / params.max_steering, -1.0, 1.0)
    return np.stack([r9[0], r9[1], r9[2], r9[3], sv, np.minimum(r9[7], target - v0), r9[4], r9[5]])


def reframe(warm, out8, N):
    """The records of the previous vehicle frame in the frame of the step-1 state the plant moved the car to: x, y rotated and
    translated, psi - psi1 (cte and epsi do not depend on the frame)."""
    w = warm.copy()
    x1, y1, p1 = out8[0], out8[1], out8[2]
    c, s = np.cos(p1), np.sin(p1)
    for k in range(N - 1):
        x, y = w[22 * k] - x1, w[22 * k + 1] - y1
        w[22 * k], w[22 * k + 1], w[22 * k + 2] = x * c + y * s, y * c - x * s, w[22 * k + 2] - p1
    return w


def loop(pkg, twin, params, sc, wp, steps, opts, record):
    mem = {"warm": None, "status": None, "out8": None}

    def step(k, pose, px, py):
        warm = mem["warm"]
        if warm is not None and record == "rigid":
            warm = reframe(warm, mem["out8"], params.N)
        if record == "as it is":
            pre = twin_run(twin, params, pose, px, py, opts)["pre"]
            b = {"state": pre[:6], "coeffs": pre[6:11], "yaw_lo": pre[11], "yaw_hi": pre[12]}
            r = twin_solve_box(twin, params, b, opts, psi_box=False, warm=warm, warm_status=mem["status"])
            r["out8"] = run_post(params, pre, r["out"])
        else:
            r = twin_run(twin, params, pose, px, py, opts, warm=warm, warm_status=mem["status"])
        mem["warm"], mem["status"], mem["out8"] = r["warm"], r["status"], r["out8"]
        return r
    return closed_loop(step, sc, wp, steps, params.max_steering)


def main():
    pkg = G.load_package()
    twin = load_run_warm_twin()
    gd = os.path.join(ROOT, "tests", "golden")
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    rows = []
    for cfgname, B, steps in POPULATIONS:
        params = pkg.params_from_json(os.path.join(gd, cfgname))
        sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=122, filtered=True)
        cold = closed_loop(lambda k, pose, px, py: twin_run(twin, params, pose, px, py, pkg.warm_opts_default()), sc, wp, steps, params.max_steering)
        cold_it = int(cold["iters"][1:].sum())
        print("%s: %d cars x %d steps, cold %.2f iterations per solve, statuses %s" % (cfgname, B, steps, cold_it / cold["iters"][1:].size,
                                                                                    np.bincount(cold["status"].ravel()).tolist()), flush=True)
        for record in ("as it is", "projected", "rigid"):
            for shift in (0, 1):
                for mu in (1e-6, 1e-4):
                    opts = pkg.warm_opts_default(shift=shift, mu_init=mu)
                    rec = loop(pkg, twin, params, sc, wp, steps, opts, record)
                    ost, o8, _ = oracle_runs(cfgname, {}, rec["pose"], rec["ptsx"], rec["ptsy"])
                    d_steer, d_accel, d_other = run_differences(rec["out8"], o8, params.max_steering)
                    it = int(rec["iters"][1:].sum())
                    row = {"config": cfgname, "cars": B, "steps": steps, "record": record, "shift": shift, "mu_init": mu,
                           "iters_per_warm_solve": it / rec["iters"][1:].size, "warm_iterations": it, "cold_iterations": cold_it, "ratio": it / cold_it,
                           "status_differs_from_oracle": int((rec["status"] != ost).sum()),
                           "solves_not_faster_than_cold": int((rec["iters"][1:] >= cold["iters"][1:]).sum()),
                           "max_d_steer_rad": d_steer, "max_d_accel": d_accel, "max_d_other_rows": d_other,
                           "within_tolerance": bool(d_steer <= TOL_STEER and d_accel <= TOL_ACCEL and d_other <= TOL_TRAJ)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    # the rule: fewest total iterations over both populations among the settings without a status difference and within tolerance
    total = {}
    for r in rows:
        key = (r["record"], r["shift"], r["mu_init"])
        t = total.setdefault(key, {"record": key[0], "shift": key[1], "mu_init": key[2], "warm_iterations": 0, "clean": True})
        t["warm_iterations"] += r["warm_iterations"]
        t["clean"] = t["clean"] and r["status_differs_from_oracle"] == 0 and r["within_tolerance"]
    ranking = sorted(total.values(), key=lambda t: (not t["clean"], t["warm_iterations"]))
    print("fewest total iterations:", json.dumps(ranking[0]))
    if "--out" in sys.argv:
        json.dump({"tool": "tools/run_warm_grid.py", "rule": "fewest total iterations over both populations, no status difference", "choice": ranking[0],
                   "ranking": ranking, "rows": rows}, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
