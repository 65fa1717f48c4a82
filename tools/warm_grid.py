#!/usr/bin/env python3
"""Grid of MpcWarmOpts on the CPU build of the warm start (tests/warm_twin; no GPU): closed loops of the two populations DESIGN.md
section 6i names, every solve compared with the oracle's own cold closed loop.  Prints one JSON line per setting: iterations per
warm solve, status differences, forks, worst deviations.   python tools/warm_grid.py [--out profiles/warm_grid.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G          # noqa: E402
import oracle_lib as O               # noqa: E402
from helpers import closed_loop_report   # noqa: E402
from warm_helpers import load_warm_twin, twin_closed_loop   # noqa: E402

pkg = G.load_package()
twin = load_warm_twin()
gd = os.path.join(ROOT, "tests", "golden")
wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
POP = [("config-fast.json", 96, 25, 122), ("config-stable.json", 64, 12, 122)]
c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
rows = []
for cfgname, B, steps, seed in POP:
    params = pkg.params_from_json(os.path.join(gd, cfgname))
    sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=seed)
    _, oh, ost = O.rollout_chunk_full((cfgname, {}, c(sc["state"]), c(sc["coeffs"]), c(sc["yaw_lo"]), c(sc["yaw_hi"]), steps))
    _, _, cit = twin_closed_loop(twin, params, sc, steps, pkg.warm_opts_default(), warm_start=False)
    cold = float(cit[1:].mean())
    for shift in (1, 0):
        for mu in (1e-3, 1e-4, 1e-5, 1e-6):
            for duals in (0, 1):
                for push in (1e-6,) if (mu, duals) != (1e-4, 0) else (1e-6, 1e-4, 1e-8):
                    o = pkg.warm_opts_default(shift=shift, mu_init=mu, duals=duals, bound_push=push)
                    h, s, it = twin_closed_loop(twin, params, sc, steps, o, warm_start=True)
                    cl = closed_loop_report(h, s, oh, ost)
                    r = {"config": cfgname, "cars": B, "steps": steps, "shift": shift, "mu_init": mu, "duals": duals, "bound_push": push,
                         "iters_cold": round(cold, 3), "iters_warm": round(float(it[1:].mean()), 3), "iters_warm_max": int(it[1:].max()),
                         "status_differs": cl["status_differs"], "forks": cl["cars_on_another_local_minimum"],
                         "oracle_status_nonzero": int((ost != 0).sum()),
                         "d_steer": cl["d_steer_rad"][3], "d_accel": cl["d_accel"][3], "d_state": cl["d_state"][3]}
                    rows.append(r); print(json.dumps(r), flush=True)
if "--out" in sys.argv:
    json.dump({"tool": "tools/warm_grid.py", "rows": rows}, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
