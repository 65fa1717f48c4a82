#!/usr/bin/env python3
"""Generate tests/golden/soc_instances.npz: the instances on which IPOPT's second-order correction (SOC) matters.

The populations are SURVEY's:
  - N = 10: bench.py's survey population, lake_track_batch(65536, config-fast, stream=3, filtered="survey");
  - N = 25: config-stable.json with N = 25, dt = 0.05, 32 768 instances drawn the same way.
The hard instances are found with the CPU build of the device solver (tests/host_twin, max_soc = 0), as tools/survey_iterations.py
does: more than 22 iterations (N = 10) or 40 (N = 25), or not converged.  Each is then solved by the oracle with max_soc = 0 and
max_soc = 4; an instance is kept when the correction is accepted at least once or the status changes.  Stored per population
(prefix n10_ / n25_): state [6, n], coeffs [5, n], yaw_lo [n], yaw_hi [n], the population index, the oracle's status and
iterations at max_soc 0 and 4, its accepted corrections and its outputs (delta0, a0) at max_soc 4; plus provenance.

Run:  python tests/golden/make_soc_instances.py     (CPU only; about 5 minutes on 8 cores; needs the built oracle and twin)
"""
import ctypes as C
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

POPS = {
    "n10": dict(config="config-fast.json", over={}, B=65536, hard_iters=22),
    "n25": dict(config="config-stable.json", over=dict(N=25, dt=0.05), B=32768, hard_iters=40),
}
CHUNK = 1024


def _pkg():
    import __graft_entry__ as G
    return G.load_package()


def _params(pop):
    p = POPS[pop]
    params = _pkg().params_from_json(os.path.join(HERE, p["config"]))
    for k, v in p["over"].items():
        setattr(params, k, v)
    return params


def _twin_job(job):
    from helpers import twin_solve
    pop, part = job
    twin = C.CDLL(os.path.join(ROOT, "tests", "host_twin", "libhost_twin.so"))
    r = twin_solve(twin, _params(pop), part, want_traj=False)
    return r["status"], r["iters"]


def _oracle_job(job):
    import oracle_lib as O
    pop, st, cf, yl, yh = job
    p = POPS[pop]
    cfg = O.load_config(p["config"], **p["over"])
    res = []
    for soc in (0, 4):
        opt = O.default_options(max_soc=soc)
        for i in range(st.shape[1]):
            cfg.yaw_low, cfg.yaw_high = float(yl[i]), float(yh[i])
            s, o9, _, _, info = O.mpc_solve(cfg, st[:, i], cf[:, i], opt)
            res.append((soc, i, s, info.iterations, info.n_soc_tried, info.n_soc_accepted, o9[6], o9[7]))
    return res


def main():
    pkg = _pkg()
    wp = pkg.scenarios.load_waypoints(os.path.join(HERE, "lake_track_waypoints.csv"))
    keys = ("state", "coeffs", "yaw_lo", "yaw_hi")
    out = {}
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        for pop, p in POPS.items():
            b = pkg.scenarios.lake_track_batch(p["B"], _params(pop), wp, stream=3, filtered="survey")
            parts = [(pop, {k: np.ascontiguousarray(b[k][..., i:i + CHUNK]) for k in keys}) for i in range(0, p["B"], CHUNK)]
            r = pool.map(_twin_job, parts)
            status = np.concatenate([x[0] for x in r]); iters = np.concatenate([x[1] for x in r])
            hard = np.where((iters > p["hard_iters"]) | (status != 0))[0]
            chunks = np.array_split(hard, max(1, len(hard) // 16))
            jobs = [(pop, b["state"][:, ch].copy(), b["coeffs"][:, ch].copy(), b["yaw_lo"][ch].copy(), b["yaw_hi"][ch].copy()) for ch in chunks]
            res = pool.map(_oracle_job, jobs)
            n = len(hard)
            o = {soc: np.zeros((n, 4), dtype=np.int64) for soc in (0, 4)}
            u = {soc: np.zeros((2, n)) for soc in (0, 4)}
            pos = 0
            for ch, rr in zip(chunks, res):
                for soc, i, s, it, tried, acc, d0, a0 in rr:
                    o[soc][pos + i] = (s, it, tried, acc)
                    u[soc][:, pos + i] = (d0, a0)
                pos += len(ch)
            keep = (o[4][:, 3] > 0) | (o[4][:, 0] != o[0][:, 0])
            idx = hard[keep]
            print(pop, "hard", n, "kept", int(keep.sum()), "soc tried", int(o[4][:, 2].sum()), "accepted", int(o[4][:, 3].sum()),
                  "status max_soc 0", np.bincount(o[0][:, 0], minlength=7).tolist(), "max_soc 4", np.bincount(o[4][:, 0], minlength=7).tolist())
            for k in keys:
                out["%s_%s" % (pop, k)] = np.ascontiguousarray(b[k][..., idx])
            out[pop + "_index"] = idx.astype(np.int64)
            out[pop + "_oracle_status0"] = o[0][keep, 0].astype(np.int32)
            out[pop + "_oracle_iters0"] = o[0][keep, 1].astype(np.int32)
            out[pop + "_oracle_status4"] = o[4][keep, 0].astype(np.int32)
            out[pop + "_oracle_iters4"] = o[4][keep, 1].astype(np.int32)
            out[pop + "_oracle_soc_accepted4"] = o[4][keep, 3].astype(np.int32)
            out[pop + "_oracle_u4"] = np.ascontiguousarray(u[4][:, keep])      # (delta0, a0) of the oracle with max_soc 4
            out[pop + "_n_hard"] = np.int64(n)
    out["provenance"] = np.array(
        "tests/golden/make_soc_instances.py: lake_track_batch(B, config, stream=3, filtered='survey'); n10 = config-fast.json B=65536, "
        "n25 = config-stable.json N=25 dt=0.05 B=32768; hard = twin (max_soc 0) iterations > 22 / 40 or status != 0; kept = oracle "
        "with max_soc 4 accepts a correction or changes status")
    np.savez_compressed(os.path.join(HERE, "soc_instances.npz"), **out)


if __name__ == "__main__":
    main()
