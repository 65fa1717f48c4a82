#!/usr/bin/env python3
"""Per-instance horizon, measured: what the HORIZON build of the lane kernel costs, and what one mixed launch
gives against a launch per horizon.  65 536 lake-track instances (config-fast.json, seed 77), every variant of a part ALTERNATING in
one session, `kernel_ms` of mpc_get_stats (the solve launch between its two events), median / min / max of --reps rounds after one
warm-up round.

 (a) the price of the build: the horizon of every instance equal to the handle's N (N = 10 and N = 25) through
     mpc_solve_batch_device_horizon against the same batch through mpc_solve_batch_device_model (uniform model rows in both);
 (b) the study: horizons {10, 20, 30, 40, 50} in equal shares on ONE N = 50 handle, sorted and shuffled, against the SUM of five
     mpc_solve_batch_device_model launches on handles created with those N, each on its share.

A library without the _horizon entry points (the parent commit) is measured on the _model variants alone, so that the two sides
of (b) can each come from the commit they exist on.  Needs an MI355X.

  python tools/horizon_bench.py [--out profiles/horizon.json] [--parts ab]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G   # noqa: E402


def summary(ms):
    return {"kernel_ms_median": float(np.median(ms)), "kernel_ms_min": float(min(ms)), "kernel_ms_max": float(max(ms)), "rounds": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "horizon.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(ROOT, "tests", "golden")
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    t = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    have = hasattr(pkg.library(), "mpc_solve_batch_device_horizon")
    res = {"tool": "tools/horizon_bench.py", "config": "config-fast.json", "seed": a.seed, "reps": a.reps, "horizon_forms_in_this_library": have}

    def inputs(params, B):
        sc = pkg.scenarios.lake_track_batch(B, params, wp, seed=a.seed)
        return {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}

    def run(mpc, b, idx=None, horizon=None):
        """one launch on the instances idx (None: all) -> kernel_ms, out, status, iters"""
        cols = (lambda v: v) if idx is None else (lambda v: v[..., idx])
        B = b["state"].shape[1] if idx is None else len(idx)
        args = [t(cols(b[k])) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")]
        kw = {"model": t(pkg.scenarios.model_rows(mpc.params, B))}
        if horizon is not None:
            kw["horizon"] = t(horizon, np.int32)
        r = mpc.solve_torch(*args, **kw)
        torch.cuda.synchronize()
        st = mpc.stats()
        return float(st.kernel_ms), r, {"n_success": int(st.n_success), "iter_sum": int(st.iter_sum), "iter_max": int(st.iter_max)}

    if "a" in a.parts:
        res["a_price_of_the_build"] = {}
        for N in (10, 25):
            params = pkg.params_from_json(os.path.join(gd, "config-fast.json"), N=N)
            b = inputs(params, a.batch)
            variants = ["model"] + (["horizon_all_N"] if have else [])
            ms = {v: [] for v in variants}
            last, info = {}, {}
            with pkg.BatchedMPC(params, a.batch, device=0) as mpc:
                for rep in range(a.reps + 1):
                    for v in variants:
                        k, r, s = run(mpc, b, horizon=np.full(a.batch, N) if v != "model" else None)
                        if rep:
                            ms[v].append(k)
                        last[v], info[v] = r, s
            e = {"B": a.batch, "N": N}
            for v in variants:
                e[v] = dict(summary(ms[v]), **info[v])
            if have:
                e["horizon_over_model"] = e["horizon_all_N"]["kernel_ms_median"] / e["model"]["kernel_ms_median"]
                e["same_bits"] = {k: bool(torch.equal(last["model"][k], last["horizon_all_N"][k])) for k in ("status", "iters")}
                x, y = last["model"]["out"], last["horizon_all_N"]["out"]
                e["same_bits"]["out"] = bool(((x == y) | (x.isnan() & y.isnan())).all())
            res["a_price_of_the_build"]["N%d" % N] = e
            print(json.dumps({"a": e}), flush=True)

    if "b" in a.parts:
        Ns = (10, 20, 30, 40, 50)
        share = a.batch // len(Ns)
        B = share * len(Ns)
        params = pkg.params_from_json(os.path.join(gd, "config-fast.json"), N=50)
        b = inputs(params, B)
        hz_sorted = np.repeat(np.array(Ns, dtype=np.int32), share)
        hz_shuffled = np.random.default_rng(11).permutation(hz_sorted)
        variants = ["five_model_launches"] + (["horizon_sorted", "horizon_shuffled"] if have else [])
        ms = {v: [] for v in variants}
        per_N = {n: [] for n in Ns}
        info, last = {}, {}
        handles = {n: pkg.BatchedMPC(pkg.params_from_json(os.path.join(gd, "config-fast.json"), N=n), share, device=0) for n in Ns}
        big = pkg.BatchedMPC(params, B, device=0) if have else None
        try:
            for rep in range(a.reps + 1):
                for v in variants:
                    if v == "five_model_launches":
                        total, outs, n_ok, it = 0.0, [], 0, 0
                        for q, n in enumerate(Ns):
                            k, r, s = run(handles[n], b, idx=np.arange(q * share, (q + 1) * share))
                            total += k; outs.append(r["out"]); n_ok += s["n_success"]; it += s["iter_sum"]
                            if rep:
                                per_N[n].append(k)
                        k, r, s = total, {"out": torch.cat(outs, dim=1)}, {"n_success": n_ok, "iter_sum": it}
                    else:
                        k, r, s = run(big, b, horizon=hz_sorted if v == "horizon_sorted" else hz_shuffled)
                    if rep:
                        ms[v].append(k)
                    last[v], info[v] = r, s
        finally:
            for h in list(handles.values()) + ([big] if big is not None else []):
                h.close()
        e = {"B": B, "share": share, "handle_N": 50, "horizons": list(Ns)}
        for v in variants:
            e[v] = dict(summary(ms[v]), **info[v])
        e["five_model_launches"]["per_N_kernel_ms_median"] = {str(n): float(np.median(per_N[n])) for n in Ns}
        if have:
            base = e["five_model_launches"]["kernel_ms_median"]
            e["over_five_model_launches"] = {v: e[v]["kernel_ms_median"] / base for v in variants}
            x, y = last["five_model_launches"]["out"], last["horizon_sorted"]["out"]
            e["sorted_wrote_the_bits_of_the_five_launches"] = bool(((x == y) | (x.isnan() & y.isnan())).all())
        res["b_the_study_in_one_launch"] = e
        print(json.dumps({"b": e}), flush=True)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
