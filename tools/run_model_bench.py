#!/usr/bin/env python3
"""Latency of one telemetry message batch through the host entry points, with and without per-instance model values (DESIGN.md
section 6k, "run() and the telemetry handler"): mpc_telemetry_batch_host against mpc_telemetry_batch_host_model on a handle as
created by default (B <= wave_max_batch: the wave kernels) and on a handle with wave_max_batch = -1 (the lane kernel, what a model
call took before the run() path had its own forms), at B = 1, 8 and 64, with uniform columns (the handle's values: the plain call's
problems) and with the columns of tests/model_helpers.py: draw_rows.  Medians of --calls calls after --warmup calls, a host clock
around the call (the host forms synchronise).  One JSON line per measurement; needs an MI355X.

  python tools/run_model_bench.py [--out profiles/run_model.json]        (--out appends the lines to the file's "rows")
  python tools/run_model_bench.py --root <another checkout, built> --plain-only --tag parent    # the same plain call on another build
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are measured")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="config-fast.json")
    ap.add_argument("--plain-only", action="store_true", help="only mpc_telemetry_batch_host (a build without the model forms)")
    ap.add_argument("--tag", default="this build")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from model_helpers import MODEL_FIELDS, draw_rows
    import __graft_entry__ as G
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    lib = pkg.library()
    gd = os.path.join(HERE, "tests", "golden")
    params = pkg.params_from_json(os.path.join(gd, a.config))
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    v = lambda x: C.c_void_p(x.ctypes.data)
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    def timed(call):
        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        ts = 1e3 * np.array(ts)
        return {"ms_median": float(np.median(ts)), "ms_p10": float(np.quantile(ts, 0.1)), "ms_p90": float(np.quantile(ts, 0.9)), "ms_min": float(ts.min())}
    for B in [int(x) for x in a.batches.split(",") if x]:
        sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=77)
        f = lambda x: np.ascontiguousarray(x, dtype=np.float64)
        pose, px, py = f(sc["pose"]), f(sc["ptsx"]), f(sc["ptsy"])
        tel = f(np.stack([pose[0], pose[1], pose[2], pose[3] * 3600.0 / 1609.34, -pose[4], np.full(B, 0.3)]))
        # two sets of columns: every column the handle's own values (the same problems as the plain call: the price of the MODEL
        # builds), and draw_rows(params, B, seed=9) of tests/model_helpers.py (other problems: cars above their own speed limit are
        # refused at set-up, and a call lasts as long as its slowest car)
        uniform = f(np.repeat(np.array([[getattr(params, k)] for k in MODEL_FIELDS]), B, axis=1))
        drawn = f(draw_rows(params, B, seed=9))
        cmd = np.zeros((2, B)); st = np.zeros(B, dtype=np.int32)
        base = {"tool": "tools/run_model_bench.py", "tag": a.tag, "config": a.config, "B": B, "calls": a.calls, "warmup": a.warmup}
        lane_params = params.copy(); lane_params.wave_max_batch = -1
        for name, p in (("default handle", params), ("wave_max_batch = -1", lane_params)):
            with pkg.BatchedMPC(p, B, device=0) as mpc:
                plain = lambda: lib.mpc_telemetry_batch_host(mpc._h, B, B, 6, v(tel), 0.02, v(px), v(py), v(cmd), v(st))
                assert plain() == 0, lib.mpc_last_error()
                emit(dict(base, handle=name, call="mpc_telemetry_batch_host", non_success=int((st != 0).sum()), **timed(plain)))
                if a.plain_only:
                    continue
                ref_cmd, ref_st = cmd.copy(), st.copy()
                for columns, model in (("uniform", uniform), ("draw_rows", drawn)):
                    mdl = lambda: lib.mpc_telemetry_batch_host_model(mpc._h, B, B, 6, v(tel), 0.02, v(px), v(py), v(model), v(cmd), v(st))
                    assert mdl() == 0, lib.mpc_last_error()
                    same = bool(np.array_equal(cmd, ref_cmd) and np.array_equal(st, ref_st)) if columns == "uniform" else None
                    emit(dict(base, handle=name, call="mpc_telemetry_batch_host_model", columns=columns, non_success=int((st != 0).sum()),
                              bitwise_the_plain_call=same, **timed(mdl)))
                # once more, plain and uniform columns alternating call by call: what the order of the blocks above contributes
                mdl = lambda: lib.mpc_telemetry_batch_host_model(mpc._h, B, B, 6, v(tel), 0.02, v(px), v(py), v(uniform), v(cmd), v(st))
                both = {"plain": [], "model": []}
                for k in range(a.warmup + a.calls):
                    for key, fn in (("plain", plain), ("model", mdl)):
                        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
                        if k >= a.warmup:
                            both[key].append(1e3 * dt)
                emit(dict(base, handle=name, call="alternating", columns="uniform", plain_ms_median=float(np.median(both["plain"])),
                          model_ms_median=float(np.median(both["model"]))))
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/run_model_bench.py", "rows": []}
        doc["rows"] += lines
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
