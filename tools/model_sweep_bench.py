#!/usr/bin/env python3
"""Per-instance model values, measured at B = 65 536, N = 10, config-fast.json:

 (a) the price of the MODEL build: the model entry point with uniform rows against the plain entry point on a handle that launches
     the same thing otherwise -- tail_cut = 0 and MPC_TAKE_ORDER=0, so both calls are one launch of the single-phase fp64 lane
     kernel over the instances in their order.  The two calls ALTERNATE on one handle; whether they wrote the same bits is recorded.
 (b) a four-value dt sweep as ONE model launch of 65 536 (a quarter of the instances per value) against four handles of 16 384,
     one per value, on four streams -- with the handles as a user gets them (deferred tails, take order; waited for with
     tail_wait) and with tail_cut = 0.

Each figure is the median of --reps rounds after one warm-up round, a host clock around a device synchronise.  Needs an MI355X.

  python tools/model_sweep_bench.py [--out profiles/model_sweep.json]
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


def stats(times):
    return {"ms_median": 1e3 * float(np.median(times)), "ms_min": 1e3 * float(min(times)), "ms_max": 1e3 * float(max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dts", default="0.05,0.08,0.1,0.15")
    ap.add_argument("--seed", type=int, default=122)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_sweep.json"))
    a = ap.parse_args()
    os.environ["MPC_TAKE_ORDER"] = "0"          # (read when a handle is created; part (b)'s default handles get it back)
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, "config-fast.json"))
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    B = a.batch
    sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=a.seed)
    ins = [t(sc[k]) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")]
    res = {"tool": "tools/model_sweep_bench.py", "config": "config-fast.json", "N": int(params.N), "B": B, "seed": a.seed, "reps": a.reps}

    # ---- (a) ----
    p0 = params.copy(); p0.tail_cut = 0
    uni = t(pkg.scenarios.model_rows(p0, B))
    with pkg.BatchedMPC(p0, B, device=0) as mpc:
        outs = {False: mpc.alloc_outputs(B, dev, True), True: mpc.alloc_outputs(B, dev, True)}
        times = {False: [], True: []}; kernel = {False: [], True: []}
        for rep in range(a.reps + 1):
            for model in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mpc.solve_torch(*ins, outputs=outs[model], model=uni if model else None)
                torch.cuda.synchronize()
                if rep:
                    times[model].append(time.perf_counter() - t0)
                    kernel[model].append(mpc.stats().kernel_ms * 1e-3)
        same = {k: bool(torch.equal(outs[False][k], outs[True][k])) for k in ("status", "iters")}
        for k in ("out", "traj"):
            x, y = outs[False][k], outs[True][k]
            same[k] = bool(((x == y) | (x.isnan() & y.isnan())).all())
        res["a_price_of_the_build"] = {"handle": "tail_cut = 0, MPC_TAKE_ORDER=0", "plain": stats(times[False]), "model_uniform_rows": stats(times[True]),
                                       "plain_kernel": stats(kernel[False]), "model_kernel": stats(kernel[True]),
                                       "model_over_plain": float(np.median(times[True]) / np.median(times[False])),
                                       "model_over_plain_kernel": float(np.median(kernel[True]) / np.median(kernel[False])),
                                       "bitwise_equal": same, "not_converged": int((outs[True]["status"] != 0).sum())}
    print(json.dumps(res["a_price_of_the_build"]), flush=True)

    # ---- (b) ----
    dts = [float(x) for x in a.dts.split(",")]
    Q = B // len(dts)
    rows = pkg.scenarios.model_rows(params, B)
    for q, dt in enumerate(dts):
        rows[0, q * Q:(q + 1) * Q] = dt
    rows_t = t(rows)
    with pkg.BatchedMPC(p0, B, device=0) as mpc:
        out1 = mpc.alloc_outputs(B, dev, True)
        one = []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mpc.solve_torch(*ins, outputs=out1, model=rows_t)
            torch.cuda.synchronize()
            if rep:
                one.append(time.perf_counter() - t0)
    b = {"dts": dts, "one_model_launch": stats(one), "one_model_launch_not_converged": int((out1["status"] != 0).sum()),
         "iters_per_solve": float(out1["iters"].double().mean())}
    part = [[x[..., q * Q:(q + 1) * Q].contiguous() for x in ins] for q in range(len(dts))]
    for name, tail_cut, order in (("four_handles_default", None, None), ("four_handles_tail_cut_0", 0, "0")):
        if order is None:
            os.environ.pop("MPC_TAKE_ORDER", None)
        else:
            os.environ["MPC_TAKE_ORDER"] = order
        hs = []
        for dt in dts:
            p = params.copy(); p.dt = dt
            if tail_cut is not None:
                p.tail_cut = tail_cut
            hs.append(pkg.BatchedMPC(p, Q, device=0))
        ss = [torch.cuda.Stream(device=dev) for _ in dts]
        outs = [h.alloc_outputs(Q, dev, True) for h in hs]
        four = []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for q, h in enumerate(hs):
                h.solve_torch(*part[q], outputs=outs[q], stream=ss[q])
            for h in hs:
                h.tail_wait()
            torch.cuda.synchronize()
            if rep:
                four.append(time.perf_counter() - t0)
        agree = all(bool(torch.equal(outs[q]["status"], out1["status"][q * Q:(q + 1) * Q])) for q in range(len(dts)))
        d_steer = max(float((outs[q]["out"][6] - out1["out"][6, q * Q:(q + 1) * Q]).abs().nan_to_num(0.0).max()) for q in range(len(dts)))
        b[name] = dict(stats(four), same_status_as_the_model_launch=agree, max_abs_d_steer_vs_model_launch=d_steer)
        for h in hs:
            h.close()
    b["one_launch_over_four_default_handles"] = b["one_model_launch"]["ms_median"] / b["four_handles_default"]["ms_median"]
    res["b_dt_sweep"] = b
    print(json.dumps(b), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
