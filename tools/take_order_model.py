#!/usr/bin/env python3
"""How many wave-passes the bulk launch would spend if it took its instances in order of predicted work.

The test-only host build of the solver header (tests/host_twin) gives every instance's number of passes (Solver::step calls:
start-up, backtracking, regularisation and a restart count as the kernel counts them).  The take order is cut into waves of 64;
a wave lives until at most `tail_few` (4) of its lanes still run, not before pass 8 (kTailFewFrom) and not beyond `tail_cut` (20):
section 6c's model.  Reported per population, each by modelled bulk wave-passes and by the instances handed to the tail slices:
the identity order, the order sorted by the TRUE pass count (the bound, not buildable), and the take-order key of
csrc/mpc_take_key.h, hardest bin first and easiest bin first.  The key is evaluated through its own source compiled for the CPU
(tests/cpp/take_key_host.cpp).

  python tools/take_order_model.py                 evaluate the committed key, write profiles/take_order_model.json
  python tools/take_order_model.py --fit           fit the tree again (needs scikit-learn) on survey streams 7 and 11, rewrite the
                                                   tables in csrc/mpc_take_key.h, then evaluate
  --cache DIR                                      keep / reuse the pass counts (a minute of CPU per population)

Populations: survey and filtered, N = 10, config-fast.json.  Stream 3 is the batch bench.py re-submits: it and stream 19 are only
ever evaluated on.  CPU only."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "carnd-mpc-project_amd", "csrc", "mpc_take_key.h")
B = 65536
FIT = (("survey", 7), ("survey", 11))
EVAL = (("survey", 3), ("survey", 19), ("filtered", 3), ("filtered", 7))
GATE = 0.90
TAIL_FEW, TAIL_CUT, TAIL_FEW_FROM = 4, 20, 8
FEATS = ("v0", "abs_epsi0", "cte0", "psi_lo", "psi_hi", "heading_L", "heading_L2", "y_L2", "over", "under")


def _params_and_waypoints():
    import __graft_entry__ as G
    pkg = G.load_package()
    gd = os.path.join(ROOT, "tests", "golden")
    return pkg, pkg.params_from_json(os.path.join(gd, "config-fast.json")), pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))


def population(job):
    """inputs and per-instance passes / iterations of one (population, stream)"""
    pop, stream, cache = job
    path = os.path.join(cache, "take_order_%s_%d.npz" % (pop, stream)) if cache else None
    if path and os.path.exists(path):
        d = np.load(path)
        return {k: d[k] for k in d.files}
    pkg, p, wp = _params_and_waypoints()
    tw = C.CDLL(os.path.join(ROOT, "tests", "host_twin", "libhost_twin.so"))
    b = pkg.scenarios.lake_track_batch(B, p, wp, stream=stream, filtered={"filtered": True, "survey": "survey"}[pop])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    d = {"state": f(b["state"]), "coeffs": f(b["coeffs"]), "yaw_lo": f(b["yaw_lo"]), "yaw_hi": f(b["yaw_hi"])}
    counts = np.zeros((B, 4), dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = tw.mpc_host_twin_traffic(C.byref(p), C.c_int64(B), C.c_int64(B), vp(d["state"]), vp(d["coeffs"]), vp(d["yaw_lo"]), vp(d["yaw_hi"]), None, vp(counts))
    assert rc == 0
    d["passes"], d["iters"] = counts[:, 2].copy(), counts[:, 3].copy()
    if path:
        np.savez(path, **d)
    return d


def build_key_host():
    """csrc/mpc_take_key.h compiled for the CPU"""
    out = os.path.join(tempfile.mkdtemp(prefix="take_key_"), "libtake_key_host.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                           "-I" + os.path.dirname(HEADER), "-o", out, os.path.join(ROOT, "tests", "cpp", "take_key_host.cpp")])
    L = C.CDLL(out)
    L.mpc_take_key_host.argtypes = [C.c_double, C.c_int64, C.c_int64] + [C.c_void_p] * 6
    L.mpc_take_key_host.restype = None
    return L


def key_of(L, horizon_s, d):
    n = len(d["yaw_lo"])
    feat = np.zeros((n, L.mpc_take_key_feats_n()), dtype=np.float32)
    bins = np.zeros(n, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L.mpc_take_key_host(horizon_s, n, n, vp(d["state"]), vp(d["coeffs"]), vp(d["yaw_lo"]), vp(d["yaw_hi"]), vp(feat), vp(bins))
    return feat, bins


def model(passes, order, few=TAIL_FEW):
    """(bulk wave-passes, mean wave life, instances handed to the slices) of a take order"""
    P = passes[order].reshape(-1, 64)
    s = -np.sort(-P, axis=1)
    life = np.minimum(s[:, 0], TAIL_CUT)
    if few > 0:
        life = np.minimum(np.where(s[:, few] >= TAIL_FEW_FROM, s[:, few], np.minimum(s[:, 0], TAIL_FEW_FROM)), TAIL_CUT)
    return {"wave_passes": int(life.sum()), "mean_wave_life": float(life.mean()), "handed_to_slices": int((P > life[:, None]).sum())}


def fit(L, horizon_s, data):
    from sklearn.tree import DecisionTreeRegressor
    X = np.concatenate([key_of(L, horizon_s, data[j])[0] for j in FIT])
    y = np.concatenate([np.minimum(data[j]["passes"], TAIL_CUT) for j in FIT]).astype(np.float64)
    nb = L.mpc_take_key_bins_n()
    t = DecisionTreeRegressor(max_leaf_nodes=nb, max_depth=6, min_samples_leaf=200, random_state=0).fit(X, y).tree_
    inner = [n for n in range(t.node_count) if t.children_left[n] >= 0]
    leaves = [n for n in range(t.node_count) if t.children_left[n] < 0]
    assert len(leaves) == nb and len(inner) == nb - 1 and inner[0] == 0
    rank = {n: r for r, n in enumerate(sorted(leaves, key=lambda n: -t.value[n, 0, 0]))}      # bin 0 = most passes predicted
    idx = {n: k for k, n in enumerate(inner)}
    kid = lambda n: idx[n] if n in idx else -1 - rank[n]
    imp = t.compute_feature_importances()
    lines = ["/* BEGIN FITTED TABLES (tools/take_order_model.py --fit) */",
             "/* importance: " + ", ".join("%s %.2f" % (FEATS[q], imp[q]) for q in np.argsort(-imp) if imp[q] >= 0.005) + " */",
             "constexpr int8_t kTakeFeat[kTakeNodes] = {" + ", ".join("%d" % t.feature[n] for n in inner) + "};",
             "constexpr float kTakeThr[kTakeNodes] = {" + ", ".join("%.9gf" % np.float32(t.threshold[n]) for n in inner) + "};",
             "constexpr int8_t kTakeKid[kTakeNodes][2] = {" + ", ".join("{%d, %d}" % (kid(t.children_left[n]), kid(t.children_right[n])) for n in inner) + "};",
             "/* mean passes (capped at the cut) of the fit's instances per bin: " + " ".join("%.1f" % t.value[n, 0, 0] for n in sorted(leaves, key=lambda n: rank[n])) + " */",
             "/* END FITTED TABLES */"]
    src = open(HEADER).read()
    src = re.sub(r"/\* BEGIN FITTED TABLES.*?/\* END FITTED TABLES \*/", lambda m: "\n".join(lines), src, flags=re.S)
    open(HEADER, "w").write(src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "take_order_model.json"))
    args = ap.parse_args()
    if args.cache:
        os.makedirs(args.cache, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host_twin")])
    _, p, _ = _params_and_waypoints()
    horizon_s = p.N * p.dt
    jobs = [(pop, s, args.cache) for pop, s in FIT + EVAL]
    with multiprocessing.get_context("spawn").Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        data = dict(zip(FIT + EVAL, pool.map(population, jobs)))
    L = build_key_host()
    if args.fit:
        fit(L, horizon_s, data)
        L = build_key_host()
    out = {"batch": B, "N": int(p.N), "config": "config-fast.json", "bins": L.mpc_take_key_bins_n(), "fitted_on": ["%s stream %d" % j for j in FIT],
           "model": {"tail_few": TAIL_FEW, "tail_cut": TAIL_CUT, "tail_few_from": TAIL_FEW_FROM}, "gate": GATE, "populations": {}}
    ok = True
    for j in FIT + EVAL:
        d = data[j]
        passes = d["passes"]
        _, bins = key_of(L, horizon_s, d)
        ident = np.arange(len(passes))
        r = {"held_out": j in EVAL, "mean_passes": float(passes.mean()), "mean_iterations": float(d["iters"].mean()),
             "identity_no_hand_over": model(passes, ident, few=0), "identity": model(passes, ident),
             "sorted_by_true_passes_bound": model(passes, np.argsort(-passes, kind="stable")),
             "key_hardest_first": model(passes, np.argsort(bins, kind="stable")),
             "key_easiest_first": model(passes, np.argsort(-bins, kind="stable")),
             "lower_limit_all_lanes_busy": float(np.minimum(passes, TAIL_CUT).sum() / 64.0),
             "bin_counts": np.bincount(bins, minlength=L.mpc_take_key_bins_n()).tolist(),
             "bin_mean_passes": [round(float(np.minimum(passes[bins == b], TAIL_CUT).mean()), 2) if (bins == b).any() else None for b in range(L.mpc_take_key_bins_n())]}
        for k in ("sorted_by_true_passes_bound", "key_hardest_first", "key_easiest_first"):
            r[k]["of_identity"] = round(r[k]["wave_passes"] / r["identity"]["wave_passes"], 4)
        if j in EVAL and j[0] == "survey":
            ok = ok and max(r["key_hardest_first"]["of_identity"], r["key_easiest_first"]["of_identity"]) <= GATE
        out["populations"]["%s_stream_%d" % j] = r
    out["gate_met_on_held_out_survey_streams"] = bool(ok)
    json.dump(out, open(args.out, "w"), indent=1)
    for k, r in out["populations"].items():
        print("%-20s identity %d (%.1f; %.1f without hand-over)  bound %.3f  key hardest-first %.3f (%d handed)  easiest-first %.3f (%d handed; identity %d)" % (
            k, r["identity"]["wave_passes"], r["identity"]["mean_wave_life"], r["identity_no_hand_over"]["mean_wave_life"],
            r["sorted_by_true_passes_bound"]["of_identity"], r["key_hardest_first"]["of_identity"], r["key_hardest_first"]["handed_to_slices"],
            r["key_easiest_first"]["of_identity"], r["key_easiest_first"]["handed_to_slices"], r["identity"]["handed_to_slices"]))
    print("gate (%.2f of identity on the held-out survey streams): %s" % (GATE, "met" if ok else "NOT met"))


if __name__ == "__main__":
    main()
