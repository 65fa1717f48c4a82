#!/usr/bin/env python3
"""Closed loops with per-instance model values, measured: the four-value dt sweep of tools/model_sweep_bench.py
as closed loops -- 65 536 cars x 25 steps, N = 10, config-fast.json, a quarter of the cars per dt -- in the four forms the library has:

 (a) mpc_rollout_batch_device_model          stepwise, cold   (the yardstick: the only form a library without the others has)
 (b) mpc_rollout_batch_device_warm_model     stepwise, warm
 (c) mpc_rollout_batch_device_fused_model    one launch, cold
 (d) mpc_rollout_batch_device_fused_model    one launch, warm

The forms ALTERNATE on one handle, each from a fresh copy of the start states; every figure is the median of --reps rounds after one
warm-up round, a host clock around a device synchronise.  The iteration sums are recorded, and whether (c) and (d) wrote the bits of
(a) and (b) into hist, state, status and iters.  A library without (b)-(d) is measured on (a) alone.  Needs an MI355X.

  python tools/model_rollout_bench.py [--out profiles/model_rollout.json]
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

FORMS = (("a_stepwise_cold", False, False), ("b_stepwise_warm", True, False), ("c_fused_cold", False, True), ("d_fused_warm", True, True))


def stats(times):
    return {"ms_median": 1e3 * float(np.median(times)), "ms_min": 1e3 * float(min(times)), "ms_max": 1e3 * float(max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dts", default="0.05,0.08,0.1,0.15")
    ap.add_argument("--seed", type=int, default=122)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_rollout.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, "config-fast.json"))
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    B, steps = a.batch, a.steps
    sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=a.seed)
    state0, coeffs, ylo, yhi = (t(sc[k]) for k in ("state", "coeffs", "yaw_lo", "yaw_hi"))
    dts = [float(x) for x in a.dts.split(",")]
    Q = B // len(dts)
    rows = pkg.scenarios.model_rows(params, B)
    for q, dt in enumerate(dts):
        rows[0, q * Q:(q + 1) * Q] = dt
    rows_t = t(rows)
    have = hasattr(pkg.library(), "mpc_rollout_batch_device_fused_model")
    forms = FORMS if have else FORMS[:1]
    res = {"tool": "tools/model_rollout_bench.py", "config": "config-fast.json", "N": int(params.N), "B": B, "steps": steps, "dts": dts,
           "seed": a.seed, "reps": a.reps, "forms_in_this_library": [f[0] for f in forms]}
    times = {f[0]: [] for f in forms}
    last = {}
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        for rep in range(a.reps + 1):
            for name, warm_start, fused in forms:
                state = state0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kw = dict(warm_start=warm_start, fused=fused) if have else {}
                r = mpc.rollout_torch(state, coeffs, ylo, yhi, steps=steps, model=rows_t, **kw)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                last[name] = {"hist": r["hist"], "state": state, "status": r["status"], "iters": r["iters"]}
        res["rollout_fused_info"] = mpc.rollout_fused_info()
    for name, _, _ in forms:
        x = last[name]
        res[name] = dict(stats(times[name]), iter_sum=int(x["iters"].long().sum()), iters_per_solve=float(x["iters"].double().mean()) / steps,
                         cars_not_success=int((x["status"] != 0).sum()))
    if have:
        def same(p, q):
            out = {k: bool(torch.equal(last[p][k], last[q][k])) for k in ("status", "iters")}
            for k in ("hist", "state"):
                x, y = last[p][k], last[q][k]
                out[k] = bool(((x == y) | (x.isnan() & y.isnan())).all())
            return out
        res["c_wrote_the_bits_of_a"] = same("c_fused_cold", "a_stepwise_cold")
        res["d_wrote_the_bits_of_b"] = same("d_fused_warm", "b_stepwise_warm")
        base = res["a_stepwise_cold"]["ms_median"]
        res["over_a"] = {name: res[name]["ms_median"] / base for name, _, _ in forms}
        res["warm_over_cold_iterations"] = res["b_stepwise_warm"]["iter_sum"] / res["a_stepwise_cold"]["iter_sum"]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
