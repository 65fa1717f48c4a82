#!/usr/bin/env python3
"""Track driving (include/mpc_amd_drive.h) against the loop a caller had to write before it: B cars x --steps
telemetry messages, config-fast, cold and warm,

  stepwise   mpc_drive_batch_device: window, handler and plant on the device, no host round trip, a launch sequence per message
  fused      mpc_drive_batch_device_fused: the same in one launch, every car advancing on its own (and whether it wrote the same bits)
  host_loop  mpc_telemetry_batch_device(_warm) once per message, with the waypoint window and the plant in numpy on the host (the
             rule of tests/run_warm_helpers.py's pick_window; the plant is the drive loop's own, restated in numpy) -- what the
             parent commit offers: one copy of the cars down and one of the windows up per message

Each figure is the median of --reps runs after --warmup runs, timed
between two events on the stream; the iteration counts of the stepwise run's records say what the slowest car of a step costs.
Writes --out (default profiles/drive.json); needs an MI355X."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G   # noqa: E402
from drive_helpers import numpy_plant as plant   # noqa: E402  (the drive loop's plant, vectorised)
from run_warm_helpers import pick_window   # noqa: E402  (the window rule the callers' loops used)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="config-fast.json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drive.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, a.config))
    wp = np.asarray(pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv")), dtype=np.float64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    B, steps = a.batch, a.steps
    car0 = pkg.scenarios.track_starts(B, params, wp, seed=122)
    d_car0, d_tx, d_ty = t(car0), t(wp[:, 0]), t(wp[:, 1])
    rows = []

    def timed(fn):
        ms = []
        for rep in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms, out
    for warm in (0, 1):
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            opts = mpc.drive_opts(warm_start=warm)
            ms_f, res_f = timed(lambda: mpc.drive_torch(d_car0.clone(), d_tx, d_ty, steps, opts=opts, fused=True))
            ms, res = timed(lambda: mpc.drive_torch(d_car0.clone(), d_tx, d_ty, steps, opts=opts))
            same = all(torch.equal(res[k].view(torch.int64) if res[k].dtype == torch.float64 else res[k],
                                   res_f[k].view(torch.int64) if res_f[k].dtype == torch.float64 else res_f[k]) for k in ("car", "summary", "hist", "status", "iters"))
            info = mpc.drive_info()
            it = res["hist"][:, 11].cpu().numpy()
            st = res["hist"][:, 10].cpu().numpy()
            summ = res["summary"].cpu().numpy()
            rows.append({"form": "stepwise", "warm_start": warm, "B": B, "steps": steps, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)),
                         "ms_max": float(max(ms)), "reps": a.reps, "warmup": a.warmup, "solves_per_s": B * steps / (1e-3 * float(np.median(ms))),
                         "iters_per_solve_step_1": float(it[0].mean()), "iters_per_solve_steps_2_on": float(it[1:].mean()) if steps > 1 else None,
                         "slowest_solve_iterations_per_step": [int(x) for x in it.max(1)],
                         "sum_over_steps_of_the_slowest": int(it.max(1).sum()), "slowest_car_iterations": int(it.sum(0).max()),
                         "mean_car_iterations": float(it.sum(0).mean()), "non_success_solves": int((st != 0).sum()),
                         "max_abs_cte_p50_p99_max": [float(np.quantile(summ[0], q)) for q in (0.5, 0.99, 1.0)],
                         "progress_waypoints_mean": float(summ[5].mean())})
            print(json.dumps(rows[-1]), flush=True)
            rows.append({"form": "fused", "warm_start": warm, "B": B, "steps": steps, "ms_median": float(np.median(ms_f)), "ms_min": float(min(ms_f)),
                         "ms_max": float(max(ms_f)), "reps": a.reps, "warmup": a.warmup, "solves_per_s": B * steps / (1e-3 * float(np.median(ms_f))),
                         "speedup_over_stepwise": float(np.median(ms) / np.median(ms_f)), "bitwise_equal_to_stepwise": bool(same), "drive_info": info})
            print(json.dumps(rows[-1]), flush=True)
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            opts = mpc.drive_opts(warm_start=warm)
            wbuf = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=dev)
            status = torch.empty((B,), dtype=torch.int32, device=dev)

            def host_loop():
                car = car0.copy()
                for k in range(steps):
                    px, py = pick_window(wp, car[0], car[1], opts.npts)
                    kw = dict(warm=wbuf if k else None, warm_status=status if k else None, warm_out=wbuf, status_out=status) if warm else {}
                    r = mpc.telemetry_torch(t(car), t(px), t(py), extra_latency=opts.extra_latency, **kw)
                    car = plant(car, r["cmd"].cpu().numpy(), params, opts.sub_old, opts.sub_new, opts.h)
                return car
            ms, car = timed(host_loop)
            rows.append({"form": "host_loop", "what": "mpc_telemetry_batch_device%s per message, window and plant in numpy on the host" % ("_warm" if warm else ""),
                         "warm_start": warm, "B": B, "steps": steps, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                         "reps": a.reps, "warmup": a.warmup, "solves_per_s": B * steps / (1e-3 * float(np.median(ms))),
                         "max_abs_difference_of_the_final_cars_to_stepwise": float(np.nanmax(np.abs(car - res["car"].cpu().numpy())))})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"tool": "tools/drive_bench.py", "config": a.config, "device": torch.cuda.get_device_name(0), "timing": "median of reps runs after warmup runs, between two events",
           "rows": rows}
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
