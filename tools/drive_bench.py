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
Writes --out (default profiles/drive.json); needs an MI355X.

--model: the mpc_drive_*_model entry points instead (default --out profiles/drive_model.json) --
  model      the stepwise and the one-launch form with every column the handle's own values (scenarios.model_rows), cold and warm,
  no_model   the same calls without `model` in the same process, and whether the two wrote the same bits (--parent FILE: the rows a
             run of this tool on the parent commit wrote in the same session are copied in beside them),
  sweep      one drive with real variation: --speeds values of max_speed x --cars cars in ONE warm one-launch call of --sweep-steps
             messages, every value on the same starts -- per value: how many cars leave the road (summary row "first step off the
             road"), when, how fast they went and how far they got.

--latency: the mpc_drive_*_latency entry points (default --out profiles/drive_latency.json) --
  grid       --delays stale-command times x --comps compensated times x --cars cars (scenarios.latency_grid, the same starts in every
             cell) in ONE warm one-launch call of --sweep-steps messages: the off-track map (cars that leave the road per cell), the
             time of the launch, and the iterations per solve along both axes -- what the reference studies with `-latency N` run N
             times.

--horizon: the mpc_drive_*_horizon entry points (default --out profiles/drive_horizon.json): an N x dt grid as
the columns of one call -- horizons 5, 7, 10, 15, 20, 25 on an N = 25 handle x dt 0.05, 0.1, 0.15, 0.2 through `model` x --cars cars per
cell (the same starts in every cell), --sweep-steps messages, warm.  --legs picks what is run:
  grid       the cars sorted by horizon: the stepwise form and the one launch, timed; per cell what the drive says (summary rows 0, 3,
             6, 7: max |cte|, mean speed, cars off the road, failed steps) -- the table a user wants
  shuffled   the same batch with its columns permuted: every wave then holds every horizon and lasts as long as its longest
  uniform    every horizon 10 on an N = 10 handle against the _fused_model call on the same handle and cars: what the unstaged HORIZON
             build costs a drive
  six        what a caller can do without the _horizon forms: six _fused_model calls on six handles created with those N, each with
             its four dt values, times summed.  Needs nothing of this commit but the tool, so --root CHECKOUT measures another built
             checkout's library (the parent commit's, in the same session) with it.
--forms picks the forms of grid and shuffled (one_launch, stepwise: a stepwise run of 300 messages lasts 300 x the slowest car of each
step, so it may be given --reps and --warmup of its own in a run of its own; every leg records the reps it was timed with).
--merge FILE ...: copy the legs of files this tool wrote into --out (legs of the same name are joined).

--plant: the mpc_drive_*_plant entry points (default --out profiles/drive_plant.json) --
  grid       --ratios values of plant Lf / model Lf (0.5 .. 1.5) x --biases steering biases (-0.1 .. 0.1 rad) x --cars cars (the same
             starts in every cell) in ONE warm one-launch _fused_plant call of --sweep-steps messages: per cell max |cte| and the first
             step off the road, and the time of the launch.
  cost       with --parent CHECKOUT (the parent commit, built): what the feature costs a caller who does not use it.  The plain run
             and the --model run of this tool, each three times on the parent's library and three times on this one, alternating, every
             run a process of its own (--root); per leg the six medians of the warm one-launch form are the figures, every other form
             is recorded beside them.
--legs grid,plain,model picks what is run (default: all three; plain and model need --parent); what --out already holds is kept: a
cost leg is a list of sessions, and a run appends one.

--budget: the mpc_drive_*_budget entry points (default --out profiles/drive_budget.json) --
  grid       --budgets iteration budgets x {cold, warm} x --cars cars (the same starts in every cell) on the lake track: per start mode ONE
             one-launch _fused_budget call of --sweep-steps messages with the budgets as its columns, timed like every figure of this
             tool; beside it the same cars through the same call with budget = NULL (the _fused_plant form: what the parent commit runs);
             per budget and start mode the mean iterations per message, the share of messages the budget ended, the share of cars that
             stay within cte_limit and the median of max |cte|.  What --out already holds is kept."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:      # (before the package is imported: --root CHECKOUT measures that checkout's library)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", action="store_true", help="measure the _model entry points and run the top-speed sweep")
    ap.add_argument("--parent", default=None, help="--model: a file this tool wrote on the parent commit in the same session; --plant, --noise: the parent commit's built checkout (the cost legs)")
    ap.add_argument("--speeds", type=int, default=16)
    ap.add_argument("--cars", type=int, default=4096)
    ap.add_argument("--sweep-steps", type=int, default=300)
    ap.add_argument("--latency", action="store_true", help="run the stale-time x compensation grid of the _latency entry points")
    ap.add_argument("--delays", type=int, default=16, help="--latency: stale-command times, 0, 10, 20 ... ms")
    ap.add_argument("--comps", type=int, default=16, help="--latency: compensated times, 0, 10, 20 ... ms")
    ap.add_argument("--period", type=int, default=16, help="--latency: plant substeps (10 ms each) between two messages")
    ap.add_argument("--horizon", action="store_true", help="run the N x dt grid of the _horizon entry points")
    ap.add_argument("--legs", default="grid,shuffled,uniform,six", help="--horizon: which legs to run")
    ap.add_argument("--forms", default="one_launch,stepwise", help="--horizon: the forms of the grid and shuffled legs")
    ap.add_argument("--root", default=None, help="--horizon --legs six: another built checkout whose library is measured")
    ap.add_argument("--plant", action="store_true", help="run the Lf-ratio x steering-bias grid of the _plant entry points")
    ap.add_argument("--ratios", type=int, default=16, help="--plant: values of plant Lf / model Lf, 0.5 .. 1.5")
    ap.add_argument("--biases", type=int, default=16, help="--plant: steering biases, -0.1 .. 0.1 rad")
    ap.add_argument("--budget", action="store_true", help="run the budget x {cold, warm} grid of the _budget entry points")
    ap.add_argument("--budgets", default="1,2,3,4,5,6,8,12,50", help="--budget: the iteration budgets of the grid")
    ap.add_argument("--noise", action="store_true", help="run the sigma x seed grid of the _noise entry points (a Monte-Carlo in one call)")
    ap.add_argument("--sigmas", type=int, default=8, help="--noise: values of sigma_pos, 0 .. 1 m (sigma_psi and sigma_speed scaled with it)")
    ap.add_argument("--seeds", type=int, default=512, help="--noise: seeds per sigma")
    ap.add_argument("--noise-mph", type=float, default=40.0, help="--noise: the top speed of the drive [mph] (at the config's own no start stays on the road for 300 messages)")
    ap.add_argument("--merge", nargs="*", default=None, help="--horizon: files of this tool whose legs are copied into --out (nothing is run)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "drive_noise.json" if a.noise else "drive_budget.json" if a.budget else "drive_plant.json" if a.plant else "drive_horizon.json" if a.horizon else "drive_latency.json" if a.latency else
                                  "drive_model.json" if a.model else "drive.json")
    if a.horizon and a.merge is not None:
        doc = {"tool": "tools/drive_bench.py --horizon", "legs": {}}
        for f in a.merge:
            d = json.load(open(f))
            doc.update({k: v for k, v in d.items() if k != "legs"})
            for name, leg in d["legs"].items():
                doc["legs"].setdefault(name, {}).update(leg)
        json.dump(doc, open(a.out, "w"), indent=1)
        print("wrote", a.out)
        return
    if (a.latency or a.plant) and a.cars == 4096:
        a.cars = 16
    if a.plant:
        return plant_grid(a)
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, a.config))
    wp = np.asarray(pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv")), dtype=np.float64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    B, steps = a.batch, a.steps
    d_tx, d_ty = t(wp[:, 0]), t(wp[:, 1])
    car0 = pkg.scenarios.track_starts(B, params, wp, seed=122) if not a.horizon else None
    d_car0 = t(car0) if car0 is not None else None
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
    if a.noise:
        return noise_grid(a, pkg, gd, wp, t, d_tx, d_ty)
    if a.budget:
        return budget_grid(a, pkg, params, wp, t, timed, d_tx, d_ty)
    if a.horizon:
        return horizon_grid(a, pkg, gd, wp, t, timed, d_tx, d_ty)
    if a.latency:
        return latency_grid(a, pkg, params, wp, t, d_tx, d_ty)
    if a.model:
        return model_rows(a, pkg, params, wp, t, timed, car0, d_car0, d_tx, d_ty)
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


def model_rows(a, pkg, params, wp, t, timed, car0, d_car0, d_tx, d_ty):
    import torch
    B, steps = a.batch, a.steps
    rows = []
    bits = lambda x: x.view(torch.int64) if x.dtype == torch.float64 else x
    same = lambda p, q: all(torch.equal(bits(p[k]), bits(q[k])) for k in ("car", "summary", "hist", "status", "iters"))
    d_model = t(pkg.scenarios.model_rows(params, B))
    for warm in (0, 1):
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            opts = mpc.drive_opts(warm_start=warm)
            got = {}
            for what, model in (("no_model", None), ("model", d_model)):
                for form, fused in (("fused", True), ("stepwise", False)):
                    ms, res = timed(lambda: mpc.drive_torch(d_car0.clone(), d_tx, d_ty, steps, opts=opts, fused=fused, model=model))
                    got[what, form] = res
                    it = res["hist"][:, 11]
                    rows.append({"what": what, "form": form, "warm_start": warm, "B": B, "steps": steps, "ms_median": float(np.median(ms)),
                                 "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": a.reps, "warmup": a.warmup,
                                 "solves_per_s": B * steps / (1e-3 * float(np.median(ms))), "iters_per_solve": float(it.mean()),
                                 "non_success_solves": int((res["hist"][:, 10] != 0).sum())})
                    print(json.dumps(rows[-1]), flush=True)
            rows.append({"what": "bits", "warm_start": warm, "model_fused_equals_model_stepwise": bool(same(got["model", "fused"], got["model", "stepwise"])),
                         "uniform_model_equals_no_model": bool(same(got["model", "stepwise"], got["no_model", "stepwise"])), "drive_info": mpc.drive_info()})
            print(json.dumps(rows[-1]), flush=True)
    # the sweep: every value of max_speed on the same starts, in one call; a start is no faster than 0.9 x the car's own limit
    n_v, n_c = a.speeds, a.cars
    mph = np.linspace(40.0, params.max_speed * 3600.0 / 1609.34, n_v)
    cars = np.tile(pkg.scenarios.track_starts(n_c, params, wp, seed=123), (1, n_v))
    model = pkg.scenarios.model_rows(params, n_v * n_c)
    model[5] = np.repeat(mph * 1609.34 / 3600.0, n_c)
    cars[3] = np.minimum(cars[3], 0.9 * np.repeat(mph, n_c))
    sweep = []
    with pkg.BatchedMPC(params, n_v * n_c, device=0) as mpc:
        opts = mpc.drive_opts(warm_start=1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = mpc.drive_torch(t(cars), d_tx, d_ty, a.sweep_steps, opts=opts, fused=True, want_hist=False, model=t(model))
        e1.record()
        torch.cuda.synchronize()
        summ, st = res["summary"].cpu().numpy().reshape(8, n_v, n_c), res["status"].cpu().numpy().reshape(n_v, n_c)
        for q in range(n_v):
            off = summ[6, q]
            sweep.append({"max_speed_mph": float(mph[q]), "cars": n_c, "cars_off_the_road": int((off >= 0).sum()),
                          "first_step_off_the_road_min_median": [float(off[off >= 0].min()), float(np.median(off[off >= 0]))] if (off >= 0).any() else None,
                          "mean_speed_mph": float(summ[3, q].mean() / a.sweep_steps), "max_abs_cte_p50_p99_max": [float(np.quantile(summ[0, q], v)) for v in (0.5, 0.99, 1.0)],
                          "progress_waypoints_mean": float(summ[5, q].mean()), "cars_with_a_failed_step": int((summ[7, q] > 0).sum()),
                          "worst_status_counts": np.bincount(st[q], minlength=6).tolist()})
            print(json.dumps(sweep[-1]), flush=True)
        sweep_doc = {"values": n_v, "cars_per_value": n_c, "steps": a.sweep_steps, "call": "mpc_drive_batch_device_fused_model, warm_start = 1, hist = NULL",
                     "cte_limit": opts.cte_limit, "ms": float(e0.elapsed_time(e1)), "drive_info": mpc.drive_info(), "rows": sweep}
    doc = {"tool": "tools/drive_bench.py --model", "config": a.config, "device": torch.cuda.get_device_name(0),
           "timing": "median of reps runs after warmup runs, between two events", "rows": rows, "sweep": sweep_doc}
    if a.parent:
        doc["parent_commit_rows_same_session"] = json.load(open(a.parent))["rows"]
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def latency_grid(a, pkg, params, wp, t, d_tx, d_ty):
    import torch
    n_d, n_c, n_cars, steps = a.delays, a.comps, a.cars, a.sweep_steps
    delays_ms, comps_s = [10 * q for q in range(n_d)], [0.01 * q for q in range(n_c)]
    cells = n_d * n_c
    B = cells * n_cars
    lat = pkg.scenarios.latency_grid(B, params, delays_ms, comps_s, a.period)
    cars = np.repeat(pkg.scenarios.track_starts(n_cars, params, wp, seed=124), cells, axis=1)      # car c of every cell: the same start
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        opts = mpc.drive_opts(warm_start=1)
        run = lambda: mpc.drive_torch(t(cars), d_tx, d_ty, steps, opts=opts, fused=True, want_hist=False, latency=t(lat))
        run(); torch.cuda.synchronize()                                                           # (the first call grows the handle's rows)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = run()
        e1.record()
        torch.cuda.synchronize()
        info = mpc.drive_info()
    # column = car * cells + delay * n_c + comp
    summ = res["summary"].cpu().numpy().reshape(8, n_cars, n_d, n_c)
    iters = res["iters"].cpu().numpy().reshape(n_cars, n_d, n_c) / float(steps)
    off = (summ[6] >= 0).sum(0)
    print("cars off the road of %d, rows: stale command time 0 .. %d ms, columns: compensated time 0 .. %d ms" % (n_cars, delays_ms[-1], 10 * (n_c - 1)))
    for q in range(n_d):
        print("%4d ms  " % delays_ms[q] + " ".join("%3d" % v for v in off[q]))
    doc = {"tool": "tools/drive_bench.py --latency", "config": a.config, "device": torch.cuda.get_device_name(0),
           "call": "mpc_drive_batch_device_fused_latency, warm_start = 1, hist = NULL, one timed call after one untimed", "B": B, "steps": steps,
           "delays_ms": delays_ms, "comps_s": comps_s, "cars_per_cell": n_cars, "period_substeps": a.period, "cte_limit": opts.cte_limit,
           "ms": float(e0.elapsed_time(e1)), "solves_per_s": B * steps / (1e-3 * float(e0.elapsed_time(e1))), "drive_info": info,
           "cars_off_the_road": off.tolist(), "max_abs_cte_median": np.median(summ[0], axis=0).tolist(),
           "failed_steps_mean": summ[7].mean(0).tolist(), "iterations_per_solve": iters.mean(0).tolist(),
           "iterations_per_solve_along_the_compensation_axis": iters.mean((0, 1)).tolist(),
           "iterations_per_solve_along_the_stale_time_axis": iters.mean((0, 2)).tolist(),
           "iterations_per_solve_by_compensation_minus_stale_time_ms": {
               str(10 * d): float(np.mean([iters[:, q, q + d].mean() for q in range(n_d) if 0 <= q + d < n_c]))
               for d in range(-(n_d - 1), n_c) if any(0 <= q + d < n_c for q in range(n_d))}}
    print("one launch: %d cars x %d messages in %.1f ms; iterations per solve along the compensation axis: %s" % (
        B, steps, doc["ms"], " ".join("%.2f" % v for v in doc["iterations_per_solve_along_the_compensation_axis"])))
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def plant_grid(a):
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, a.config))
    wp = np.asarray(pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv")), dtype=np.float64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    n_r, n_b, n_cars, steps = a.ratios, a.biases, a.cars, a.sweep_steps
    ratios, biases = np.linspace(0.5, 1.5, n_r), np.linspace(-0.1, 0.1, n_b)
    cells = n_r * n_b
    B = cells * n_cars
    # column = car * cells + ratio * n_b + bias; car c of every cell: the same start
    plant = pkg.drive_plant_default(params, B)
    plant[0] = params.Lf * np.tile(np.repeat(ratios, n_b), n_cars)
    plant[2] = np.tile(np.tile(biases, n_r), n_cars)
    cars = np.repeat(pkg.scenarios.track_starts(n_cars, params, wp, seed=126), cells, axis=1)
    legs = ["grid", "plain", "model"] if a.legs == ap_default_legs else [x for x in a.legs.split(",") if x]
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.update({"tool": "tools/drive_bench.py --plant", "config": a.config, "device": torch.cuda.get_device_name(0)})
    if "grid" in legs:
        doc["grid"] = plant_grid_leg(a, pkg, params, wp, t, plant, cars, ratios, biases)
    if a.parent and ("plain" in legs or "model" in legs):
        plant_cost_legs(a, doc, legs)
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


ap_default_legs = "grid,shuffled,uniform,six"


def plant_grid_leg(a, pkg, params, wp, t, plant, cars, ratios, biases):
    import torch
    n_r, n_b, n_cars, steps = a.ratios, a.biases, a.cars, a.sweep_steps
    B = n_r * n_b * n_cars
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        opts = mpc.drive_opts(warm_start=1)
        d_tx, d_ty = t(wp[:, 0]), t(wp[:, 1])
        run = lambda: mpc.drive_torch(t(cars), d_tx, d_ty, steps, opts=opts, fused=True, want_hist=False, plant=t(plant))
        run(); torch.cuda.synchronize()                                                           # (the first call grows the handle's rows)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = run()
        e1.record()
        torch.cuda.synchronize()
        info = mpc.drive_info()
    summ = res["summary"].cpu().numpy().reshape(8, n_cars, n_r, n_b)
    off = np.where(summ[6] >= 0, summ[6], np.inf)
    first_off = off.min(0)
    print("cars off the road of %d, rows: plant Lf / model Lf %.2f .. %.2f, columns: steering bias %.3f .. %.3f rad" % (n_cars, ratios[0], ratios[-1], biases[0], biases[-1]))
    for q in range(n_r):
        print("%5.2f  " % ratios[q] + " ".join("%3d" % v for v in (summ[6, :, q] >= 0).sum(0)))
    leg = {"call": "mpc_drive_batch_device_fused_plant, warm_start = 1, hist = NULL, one timed call after one untimed", "B": B, "steps": steps,
                    "lf_ratios": ratios.tolist(), "steer_biases_rad": biases.tolist(), "cars_per_cell": n_cars, "cte_limit": opts.cte_limit,
                    "ms": float(e0.elapsed_time(e1)), "solves_per_s": B * steps / (1e-3 * float(e0.elapsed_time(e1))), "drive_info": info,
                    "max_abs_cte_max_over_cars": summ[0].max(0).tolist(), "max_abs_cte_median_over_cars": np.median(summ[0], axis=0).tolist(),
                    "first_step_off_the_road": [[None if np.isinf(v) else int(v) for v in row] for row in first_off],
                    "cars_off_the_road": (summ[6] >= 0).sum(0).tolist(), "failed_steps_mean": summ[7].mean(0).tolist()}
    print("one launch: %d cars x %d messages in %.1f ms" % (B, steps, leg["ms"]))
    return leg


def plant_cost_legs(a, doc, legs):
    import subprocess
    import tempfile
    # every run a process of its own, one at a time: the parent's library and this one, alternating
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cost = doc.setdefault("cost_of_the_unused_feature", {"legs": {}})
    cost.update({"what": "tools/drive_bench.py (plain) and --model, batch %d x %d messages; three runs on the parent commit's library and three on this "
                         "build's, alternating, every run a process of its own; ms_median of every form per run" % (a.batch, a.steps),
                 "judged_on": "the warm one-launch form (fused, warm_start = 1; --model: model, fused, warm_start = 1)"})
    with tempfile.TemporaryDirectory() as d:
        for leg, extra in (("plain", []), ("model", ["--model", "--speeds", "1", "--cars", "64", "--sweep-steps", "1"])):
            if leg not in legs:
                continue
            runs = {"parent": [], "this_build": []}
            for r in range(3):
                for who, root in (("parent", os.path.abspath(a.parent)), ("this_build", here)):
                    out = os.path.join(d, "%s_%s_%d.json" % (leg, who, r))
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--out", out, "--batch", str(a.batch), "--steps", str(a.steps),
                                    "--reps", str(a.reps), "--warmup", str(a.warmup), "--config", a.config] + extra, check=True, stdout=subprocess.DEVNULL, timeout=600)
                    rows = [x for x in json.load(open(out))["rows"] if "ms_median" in x and x.get("form") != "host_loop"]
                    runs[who].append({"%s%s_warm%d" % (x["what"] + "_" if "what" in x else "", x["form"], x["warm_start"]): x["ms_median"] for x in rows})
                    print(leg, who, r, json.dumps(runs[who][-1]), flush=True)
            key = "model_fused_warm1" if leg == "model" else "fused_warm1"
            par, new = [x[key] for x in runs["parent"]], [x[key] for x in runs["this_build"]]
            cost["legs"].setdefault(leg, []).append({"reps": a.reps, "warmup": a.warmup, "runs": runs, "figure": key, "parent_ms": par, "this_build_ms": new, "this_build_median_ms": float(np.median(new)),
                                 "parent_spread_ms": [min(par), max(par)], "median_inside_the_parent_spread": bool(min(par) <= np.median(new) <= max(par)),
                                 "median_not_above_the_parent_spread": bool(np.median(new) <= max(par))})
            print(leg, json.dumps({k: v for k, v in cost["legs"][leg][-1].items() if k != "runs"}), flush=True)


def budget_grid(a, pkg, params, wp, t, timed, d_tx, d_ty):
    import torch
    budgets = [int(x) for x in a.budgets.split(",") if x]
    n_b, n_cars, steps = len(budgets), (256 if a.cars == 4096 else a.cars), a.sweep_steps
    B = n_b * n_cars
    # column = budget * n_cars + car; car c of every budget: the same start
    cars = np.tile(pkg.scenarios.track_starts(n_cars, params, wp, seed=127), (1, n_b))
    d_budget = torch.from_numpy(np.repeat(np.array(budgets, dtype=np.int32), n_cars)).to(d_tx.device)
    d_cars = t(cars)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    grid = {"call": "mpc_drive_batch_device_fused_budget, hist given (the records say which messages the budget ended)", "B": B, "steps": steps, "budgets": budgets,
            "cars_per_budget": n_cars, "timing": "median of reps runs after warmup runs, between two events", "start_modes": {}}
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        for warm in (0, 1):
            opts = mpc.drive_opts(warm_start=warm)
            ms0, base = timed(lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=True))
            ms, res = timed(lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=True, budget=d_budget))
            hist = res["hist"].cpu().numpy().reshape(steps, 13, n_b, n_cars)
            summ = res["summary"].cpu().numpy().reshape(8, n_b, n_cars)
            bsum, bhist = base["summary"].cpu().numpy(), base["hist"].cpu().numpy()
            leg = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": a.reps, "warmup": a.warmup,
                   "budget_null_same_cars": {"what": "the same call with budget = NULL: the _fused_plant form, the wave kernels or the staged lane kernel",
                                             "ms_median": float(np.median(ms0)), "ms_min": float(min(ms0)), "ms_max": float(max(ms0)),
                                             "iterations_per_message": float(bhist[:, 11].mean()), "share_of_cars_within_cte_limit": float((bsum[6] < 0).mean()),
                                             "max_abs_cte_median": float(np.median(bsum[0]))},
                   "cte_limit": opts.cte_limit, "drive_info": mpc.drive_info(), "rows": []}
            for q, b in enumerate(budgets):
                leg["rows"].append({"budget": b, "iterations_per_message": float(hist[:, 11, q].mean()), "share_of_messages_ended_by_the_budget": float((hist[:, 10, q] == 1).mean()),
                                    "share_of_cars_within_cte_limit": float((summ[6, q] < 0).mean()), "max_abs_cte_median": float(np.median(summ[0, q])),
                                    "first_step_off_the_road_median": float(np.median(summ[6, q][summ[6, q] >= 0])) if (summ[6, q] >= 0).any() else None})
                print("warm %d" % warm, json.dumps(leg["rows"][-1]), flush=True)
            print("warm %d: %d cars x %d messages, budget grid %.1f ms, budget = NULL %.1f ms" % (warm, B, steps, leg["ms_median"], leg["budget_null_same_cars"]["ms_median"]), flush=True)
            grid["start_modes"]["warm" if warm else "cold"] = leg
    doc.update({"tool": "tools/drive_bench.py --budget", "config": a.config, "device": torch.cuda.get_device_name(0), "grid": grid})
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def noise_grid(a, pkg, gd, wp, t, d_tx, d_ty):
    """sigmas x seeds x sweep-steps messages as ONE mpc_drive_batch_device_fused_noise call, cold and warm; beside it the same cars with
    the zero column and with noise = NULL (the _fused_budget path): the zero-column time against the NULL time is the cost of the feature
    to a caller who passes the array.  --parent CHECKOUT: the plain drive on the parent commit's library and on this one, alternating (the
    --plant cost legs): what the feature costs a caller who does not.
    The drive: --config at a top speed of --noise-mph, from the one of 64 candidate starts (scenarios.track_starts, seed 127) that a
    noise-free pre-drive keeps on the road with the smallest max |cte0| -- so that FIRST_OFF == -1 at sigma 0 and the noise alone moves it."""
    import torch
    from carnd_mpc_project_amd import _abi
    n_s, n_seeds, steps = a.sigmas, a.seeds, a.sweep_steps
    B = n_s * n_seeds
    sig = np.linspace(0.0, 1.0, n_s)
    params = pkg.params_from_json(os.path.join(gd, a.config), max_speed=a.noise_mph * 1609.34 / 3600.0)
    cand = pkg.scenarios.track_starts(64, params, wp, seed=127)
    with pkg.BatchedMPC(params, 64, device=0) as mpc:
        pre = mpc.drive_torch(t(cand), d_tx, d_ty, steps, opts=mpc.drive_opts(warm_start=0), fused=True, want_hist=False)["summary"].cpu().numpy()
    on = pre[6] < 0
    assert on.any(), "no candidate start stays on the road without noise: lower --noise-mph"
    pick = int(np.argmin(np.where(on, pre[0], np.inf)))
    print("start: candidate %d of 64 (%d stay on the road without noise), max |cte0| %.3f m over %d messages" % (pick, on.sum(), pre[0, pick], steps), flush=True)
    # column = sigma * n_seeds + seed; every column: the same start (the spread is the noise's alone), seed s of every sigma: the same stream
    cars = np.tile(cand[:, pick:pick + 1], (1, B))
    noise = pkg.drive_noise_default(B, np.tile(10000 + np.arange(n_seeds), n_s))
    noise[_abi.NOISE_POS] = np.repeat(sig, n_seeds)
    noise[_abi.NOISE_PSI] = 0.05 * noise[_abi.NOISE_POS]            # 1 m goes with 0.05 rad and 2 mph
    noise[_abi.NOISE_SPEED] = 2.0 * noise[_abi.NOISE_POS]
    zero = pkg.drive_noise_default(B, noise[_abi.NOISE_SEED].astype(np.int64))
    d_cars, d_noise, d_zero = t(cars), t(noise), t(zero)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    grid = {"call": "mpc_drive_batch_device_fused_noise, hist given", "B": B, "steps": steps, "top_speed_mph": a.noise_mph,
            "start": {"candidate": pick, "of": 64, "candidates_on_the_road_without_noise": int(on.sum()), "max_abs_cte0_without_noise": float(pre[0, pick])},
            "sigma_pos_m": [float(x) for x in sig],
            "sigma_psi_rad": [float(0.05 * x) for x in sig], "sigma_speed_mph": [float(2.0 * x) for x in sig], "seeds_per_sigma": n_seeds,
            "timing": "median of reps runs after warmup runs, between two events; the three calls of a start mode alternate rep by rep", "start_modes": {}}
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        for warm in (0, 1):
            opts = mpc.drive_opts(warm_start=warm)
            calls = {"noise": lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=True, noise=d_noise),
                     "zero_column": lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=True, noise=d_zero),
                     "noise_null": lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=True)}
            ms, out = {k: [] for k in calls}, {}
            for r in range(a.warmup + a.reps):          # interleaved: a drift of the clock meets all three alike
                for k, fn in calls.items():
                    m, out[k] = timed_once(torch, fn)
                    if r >= a.warmup:
                        ms[k].append(m)
            res = out["noise"]
            hist = res["hist"].cpu().numpy().reshape(steps, 13, n_s, n_seeds)
            summ = res["summary"].cpu().numpy().reshape(8, n_s, n_seeds)
            same = all(torch.equal(out["zero_column"][k], out["noise_null"][k]) for k in ("car", "summary", "hist", "status", "iters"))
            stat = lambda v: {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))}
            leg = dict(stat(ms["noise"]), reps=a.reps, warmup=a.warmup, cte_limit=opts.cte_limit, drive_info=mpc.drive_info(),
                       zero_column_same_cars=dict(stat(ms["zero_column"]), bitwise_equal_to_noise_null=bool(same)),
                       noise_null_same_cars=dict(stat(ms["noise_null"]), what="the same call with noise = NULL: the _fused_budget path"),
                       zero_column_over_noise_null=float(np.median(ms["zero_column"]) / np.median(ms["noise_null"])),
                       noise_null_spread_max_over_min=float(max(ms["noise_null"]) / min(ms["noise_null"])), rows=[])
            for q in range(n_s):
                leg["rows"].append({"sigma_pos_m": float(sig[q]), "share_of_cars_within_cte_limit": float((summ[6, q] < 0).mean()),
                                    "first_step_off_the_road_median": float(np.median(summ[6, q][summ[6, q] >= 0])) if (summ[6, q] >= 0).any() else None,
                                    "max_abs_cte0_p50_p90_p99_max": [float(np.quantile(summ[0, q], x)) for x in (0.5, 0.9, 0.99, 1.0)],
                                    "iterations_per_message": float(hist[:, 11, q].mean()), "non_success_messages": int((hist[:, 10, q] != 0).sum())})
                print("warm %d" % warm, json.dumps(leg["rows"][-1]), flush=True)
            print("warm %d: %d cars x %d messages: noise %.1f ms, zero column %.1f ms, noise = NULL %.1f ms (min .. max %.1f .. %.1f)" % (
                warm, B, steps, leg["ms_median"], leg["zero_column_same_cars"]["ms_median"], leg["noise_null_same_cars"]["ms_median"],
                leg["noise_null_same_cars"]["ms_min"], leg["noise_null_same_cars"]["ms_max"]), flush=True)
            grid["start_modes"]["warm" if warm else "cold"] = leg
    doc.update({"tool": "tools/drive_bench.py --noise", "config": a.config, "device": torch.cuda.get_device_name(0), "grid": grid})
    if a.parent:
        doc.pop("cost_of_the_unused_feature", None)
        plant_cost_legs(a, doc, ["plain"])
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def timed_once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


HORIZON_NS, HORIZON_DTS = (5, 7, 10, 15, 20, 25), (0.05, 0.1, 0.15, 0.2)


def horizon_grid(a, pkg, gd, wp, t, timed, d_tx, d_ty):
    import torch
    dev = d_tx.device
    n_cars, steps = a.cars, a.sweep_steps
    legs = [x for x in a.legs.split(",") if x]
    cfg = os.path.join(gd, a.config)
    big = pkg.params_from_json(cfg, N=max(HORIZON_NS))
    cells = [(n, dt) for n in HORIZON_NS for dt in HORIZON_DTS]            # sorted by horizon
    B = len(cells) * n_cars
    start = pkg.scenarios.track_starts(n_cars, big, wp, seed=125)         # car c of every cell: the same start
    cars = np.tile(start, (1, len(cells)))
    model = pkg.scenarios.model_rows(big, B)
    model[0] = np.repeat([dt for _, dt in cells], n_cars)
    hz = np.repeat([n for n, _ in cells], n_cars).astype(np.int32)
    ti = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    med = lambda ms: {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": a.reps, "warmup": a.warmup}
    doc = {"tool": "tools/drive_bench.py --horizon", "config": a.config, "device": torch.cuda.get_device_name(0),
           "timing": "median of reps runs after warmup runs, between two events", "horizons": list(HORIZON_NS), "dts": list(HORIZON_DTS),
           "cars_per_cell": n_cars, "B": B, "steps": steps, "warm_start": 1, "legs": {}}

    def table(summ, st):
        out = []
        summ, st = summ.reshape(8, len(cells), n_cars), st.reshape(len(cells), n_cars)
        for q, (n, dt) in enumerate(cells):
            out.append({"N": n, "dt": dt, "max_abs_cte_p50_max": [float(np.median(summ[0, q])), float(summ[0, q].max())],
                        "mean_speed_mph": float(summ[3, q].mean() / steps), "cars_off_the_road": int((summ[6, q] >= 0).sum()),
                        "failed_steps_mean": float(summ[7, q].mean()), "cars_with_a_failed_step": int((summ[7, q] > 0).sum())})
        return out

    def both_forms(mpc, d_cars, d_model, d_hz, tag):
        opts = mpc.drive_opts(warm_start=1)
        leg = {}
        res = {}
        for form, fused in (("one_launch", True), ("stepwise", False)):
            if form not in a.forms.split(","):
                continue
            ms, res[form] = timed(lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=fused, want_hist=False, model=d_model, horizon=d_hz))
            leg[form] = dict(med(ms), solves_per_s=B * steps / (1e-3 * float(np.median(ms))), iterations_per_solve=float(res[form]["iters"].double().mean()) / steps)
            print(tag, form, json.dumps(leg[form]), flush=True)
        bits = lambda x: x.view(torch.int64) if x.dtype == torch.float64 else x
        if len(res) == 2:
            leg["one_launch_bitwise_equal_to_stepwise"] = bool(all(torch.equal(bits(res["one_launch"][k]), bits(res["stepwise"][k])) for k in ("car", "summary", "status", "iters")))
        return leg, next(iter(res.values()))
    if "grid" in legs or "shuffled" in legs:
        with pkg.BatchedMPC(big, B, device=0) as mpc:
            if "grid" in legs:
                leg, res = both_forms(mpc, t(cars), t(model), ti(hz), "grid")
                leg["cells"] = table(res["summary"].cpu().numpy(), res["status"].cpu().numpy())
                doc["legs"]["grid_sorted_by_horizon"] = leg
                for row in leg["cells"]:
                    print(json.dumps(row), flush=True)
            if "shuffled" in legs:
                perm = np.random.default_rng(7).permutation(B)
                leg, _ = both_forms(mpc, t(cars[:, perm]), t(model[:, perm]), ti(hz[perm]), "shuffled")
                doc["legs"]["grid_shuffled"] = leg
    if "uniform" in legs:
        ten = pkg.params_from_json(cfg, N=10)
        with pkg.BatchedMPC(ten, B, device=0) as mpc:
            opts = mpc.drive_opts(warm_start=1)
            d_cars, d_model, d_hz = t(cars), t(model), ti(np.full(B, 10))
            leg = {}
            for what, kw in (("fused_horizon_all_10", dict(horizon=d_hz)), ("fused_model", {})):
                ms, r = timed(lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=True, want_hist=False, model=d_model, **kw))
                leg[what] = dict(med(ms), iterations_per_solve=float(r["iters"].double().mean()) / steps)
                leg[what + "_car"] = r["car"]
                print("uniform", what, json.dumps(leg[what]), flush=True)
            leg["bitwise_equal"] = bool(torch.equal(leg.pop("fused_horizon_all_10_car").view(torch.int64), leg.pop("fused_model_car").view(torch.int64)))
            leg["drive_info"] = mpc.drive_info()
            doc["legs"]["uniform_N_10"] = leg
    if "six" in legs:
        leg = {"what": "six mpc_drive_batch_device_fused_model calls on six handles created with N = 5 .. 25, each with its four dt cells; times summed",
               "library_of": ROOT if a.root else "this checkout", "calls": []}
        for q, n in enumerate(HORIZON_NS):
            sl = slice(q * len(HORIZON_DTS) * n_cars, (q + 1) * len(HORIZON_DTS) * n_cars)
            with pkg.BatchedMPC(pkg.params_from_json(cfg, N=n), sl.stop - sl.start, device=0) as mpc:
                opts = mpc.drive_opts(warm_start=1)
                d_cars, d_model = t(cars[:, sl]), t(model[:, sl])
                ms, r = timed(lambda: mpc.drive_torch(d_cars.clone(), d_tx, d_ty, steps, opts=opts, fused=True, want_hist=False, model=d_model))
                leg["calls"].append(dict(med(ms), N=n, B=sl.stop - sl.start, iterations_per_solve=float(r["iters"].double().mean()) / steps, drive_info=mpc.drive_info()))
                print("six", json.dumps(leg["calls"][-1]), flush=True)
        leg["ms_median_summed"] = float(sum(c["ms_median"] for c in leg["calls"]))
        doc["legs"]["six_fused_model_calls" + ("_parent_commit" if a.root else "")] = leg
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
