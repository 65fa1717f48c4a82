#!/usr/bin/env python3
"""The certificate of a stored point, measured: one launch of mpc_certify_batch_device on 65 536 N = 10 records
next to `kernel_ms` of the cold solve that wrote them.  config-fast.json, lake-track instances (seed 77); the records come from one
cold mpc_solve_batch_device_warm call (warm_in = NULL); the certificate is timed between two events on its stream, median / min / max
of --reps launches after --warmup launches.  No gate: the number goes to profiles/certify.json and into DESIGN.  Needs an MI355X.

  python tools/certify_bench.py [--out profiles/certify.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    params = pkg.params_from_json(os.path.join(gd, "config-fast.json"))
    params.f64_f32_start = 0
    B = a.batch
    sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=a.seed)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    args = [t(sc[k]) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")]
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        solve_ms = []
        for _ in range(3):                                   # the cold solve that writes the records (the last one's are certified)
            r = mpc.solve_torch(*args, want_warm=True)
            torch.cuda.synchronize()
            solve_ms.append(float(mpc.stats().kernel_ms))
        status = r["status"].cpu().numpy()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for _ in range(a.warmup):
            c = mpc.certify_torch(*args, r["warm"])
        torch.cuda.synchronize()
        for e0, e1 in ev:
            e0.record()
            c = mpc.certify_torch(*args, r["warm"])
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        verdict = c["verdict"].cpu().numpy()
    read_bytes = B * ((params.N - 1) * 22 + 13) * 8
    med = float(np.median(ms))
    res = {"tool": "tools/certify_bench.py", "config": "config-fast.json", "N": int(params.N), "batch": B, "seed": a.seed,
           "certify_ms": {"median": med, "min": float(min(ms)), "max": float(max(ms)), "launches": a.reps, "warmup": a.warmup},
           "cold_solve_kernel_ms": {"median": float(np.median(solve_ms)), "all": solve_ms},
           "certify_over_solve": med / float(np.median(solve_ms)),
           "bytes_read": read_bytes, "read_GB_per_s": read_bytes / (med * 1e-3) / 1e9,
           "status_counts": np.bincount(status, minlength=7).tolist(), "verdict_counts": np.bincount(verdict, minlength=5).tolist()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
