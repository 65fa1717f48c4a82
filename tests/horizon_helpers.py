"""Helpers of the per-instance horizon tests (test infrastructure): the TEST-ONLY CPU build of the mpc_*_horizon calls
(tests/host_twin/horizon_twin.cpp, a library of its own), the stated populations, the yardsticks -- the existing twin and the
oracle with N = n_i per instance -- and the comparisons both test files make."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
from helpers import ROOT, load_golden, vp
from model_helpers import MODEL_FIELDS, draw_rows, population

WARM_REC = 22
SENTINEL = -7777.25
INFEASIBLE = 3
HORIZONS = (3, 4, 5, 7, 10, 13, 17, 25)      # the stated draw of the bitwise and oracle tests (an N = 25 handle)
LOOP_HORIZONS = (3, 4, 5, 7, 10)             # ... and of the closed loops

_twin = None


def load_horizon_twin():
    """tests/host_twin/horizon_twin.cpp -> libhorizon_twin.so, compiled by a g++ line of its own (the twin's Makefile and its
    library stay what they are)."""
    global _twin
    if _twin is None:
        d = os.path.join(ROOT, "tests", "host_twin")
        src, out = os.path.join(d, "horizon_twin.cpp"), os.path.join(d, "libhorizon_twin.so")
        csrc = os.path.join(ROOT, "carnd-mpc-project_amd", "csrc")
        deps = [src, os.path.join(csrc, "mpc_core.h"), os.path.join(ROOT, "include", "mpc_amd.h"), os.path.join(ROOT, "include", "mpc_amd_horizon.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
            tmp = out + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                                   "-I", csrc, "-o", tmp, src])
            os.replace(tmp, out)
        _twin = C.CDLL(out)
    return _twin


def draw_horizons(B=193, seed=11, choices=HORIZONS):
    return np.random.default_rng(seed).choice(list(choices), B).astype(np.int32)


def stated_population(pkg, golden_dir, waypoints, B=193):
    """config-fast.json at N = 25, the B = 193 population of model_helpers with its model rows, and the stated horizons."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), N=25)
    b, model = population(pkg, params, waypoints, B)
    return params, b, model, draw_horizons(B)


def sub_batch(b, idx):
    return {"state": np.ascontiguousarray(b["state"][:, idx]), "coeffs": np.ascontiguousarray(b["coeffs"][:, idx]),
            "yaw_lo": np.ascontiguousarray(b["yaw_lo"][idx]), "yaw_hi": np.ascontiguousarray(b["yaw_hi"][idx])}


def with_N(params, n):
    q = params.copy()
    q.N = int(n)
    return q


def twin_horizon_solve(twin, params, batch, horizon, opts=None, model=None, warm=None, warm_status=None, want_warm=False, weights=None):
    """mpc_horizon_twin_solve with the arguments of mpc_solve_batch_host_warm_horizon.  traj and warm_out hold SENTINEL before the call
    (warm_out: wherever `warm` is not given; with `warm` the call runs in separate buffers, warm_out again all SENTINEL)."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh = f(batch["state"]), f(batch["coeffs"]), f(batch["yaw_lo"]), f(batch["yaw_hi"])
    B = st.shape[1]
    N, rows = params.N, (params.N - 1) * WARM_REC
    hz = np.ascontiguousarray(horizon, dtype=np.int32)
    out = np.zeros((9, B)); traj = np.full((2 * N, B), SENTINEL); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    md = f(model) if model is not None else None
    w = f(weights) if weights is not None else None
    warm_call = warm is not None or want_warm
    wout = np.full((rows, B), SENTINEL) if warm_call else None
    if warm is not None:
        warm = f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_horizon_twin_solve(C.byref(params), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), vp(w), vp(md), vp(hz), vp(warm),
                                     vp(warm_status), vp(wout), C.c_int64(B), C.byref(opts) if opts is not None else None, vp(out), vp(traj),
                                     vp(status), vp(iters))
    assert rc == 0, rc
    return {"out": out, "traj": traj, "status": status, "iters": iters, "warm": wout}


def twin_plain_solve(twin, params, batch, opts=None, model=None, warm=None, warm_status=None, want_warm=False, weights=None):
    """The EXISTING twin (mpc_twin_solve of tests/host_twin) on a handle of params.N: the yardstick of the bitwise tests."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh = f(batch["state"]), f(batch["coeffs"]), f(batch["yaw_lo"]), f(batch["yaw_hi"])
    B = st.shape[1]
    N, rows = params.N, (params.N - 1) * WARM_REC
    out = np.zeros((9, B)); traj = np.zeros((2 * N, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    md = f(model) if model is not None else None
    w = f(weights) if weights is not None else None
    warm_call = warm is not None or want_warm
    wout = np.zeros((rows, B)) if warm_call else None
    if warm is not None:
        warm = f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_twin_solve(C.byref(params), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), vp(w), vp(md), vp(warm), vp(warm_status),
                             vp(wout), C.c_int64(B), C.byref(opts) if opts is not None else None, C.c_int(0), vp(out), vp(traj), vp(status), vp(iters))
    assert rc == 0, rc
    return {"out": out, "traj": traj, "status": status, "iters": iters, "warm": wout}


def assert_columns_equal_per_n(got, N, horizon, ref_of, what="", warm_key="warm"):
    """Every column of `got` (a call on a handle of N with `horizon`) against ref_of(n, idx) -> the result of a handle created with
    N = n on the sub-batch idx: out, status, iters, the first n trajectory points of each half and the first (n - 1) * 22 rows of the
    warm buffer bitwise; SENTINEL in every row of traj and warm outside those prefixes."""
    horizon = np.asarray(horizon)
    for n in sorted(set(int(v) for v in horizon)):
        idx = np.nonzero(horizon == n)[0]
        ref = ref_of(n, idx)
        for k in ("out", "status", "iters"):
            assert np.array_equal(got[k][..., idx], ref[k], equal_nan=True), (what, n, k, idx[:4].tolist())
        if got.get("traj") is not None:
            t = got["traj"][:, idx]
            if ref.get("traj") is not None:
                assert np.array_equal(t[:n], ref["traj"][:n], equal_nan=True) and np.array_equal(t[N:N + n], ref["traj"][n:2 * n], equal_nan=True), (what, n, "traj")
            assert (t[n:N] == SENTINEL).all() and (t[N + n:] == SENTINEL).all(), (what, n, "traj rows behind the prefix were written")
        if got.get(warm_key) is not None:
            wv = got[warm_key][:, idx]
            r = (n - 1) * WARM_REC
            if ref.get("warm") is not None:
                assert np.array_equal(wv[:r], ref["warm"][:r], equal_nan=True), (what, n, "warm_out")
            assert (wv[r:] == SENTINEL).all(), (what, n, "warm rows behind the prefix were written")


def oracle_horizon_solve(cfgname, batch, model, horizon, N, **overrides):
    """The oracle on every instance with its own OrcConfig: N = n_i, and dt, Lf and the limits of its column (model None: the
    config's).  traj comes back in the handle's shape, [2N, B], 0 outside each instance's prefix (masked_traj does the same to a result)."""
    B = batch["state"].shape[1]
    out = np.zeros((9, B)); traj = np.zeros((2 * N, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    for i in range(B):
        n = int(horizon[i])
        over = dict(overrides, N=n)
        if model is not None:
            over.update({name: float(model[q, i]) for q, name in enumerate(MODEL_FIELDS)})
        cfg = O.load_config(cfgname, **over)
        cfg.yaw_low, cfg.yaw_high = float(batch["yaw_lo"][i]), float(batch["yaw_hi"][i])
        st, o9, tx, ty, info = O.mpc_solve(cfg, batch["state"][:, i], batch["coeffs"][:, i])
        out[:, i] = o9; traj[:n, i] = tx; traj[N:N + n, i] = ty; status[i] = st; iters[i] = info.iterations
    return {"out": out, "traj": traj, "status": status, "iters": iters}


def masked_traj(res, N, horizon):
    """a copy of `res` whose traj holds 0 outside every instance's prefix on both sides of a comparison with oracle_horizon_solve"""
    t = np.array(res["traj"], copy=True)
    for i, n in enumerate(np.asarray(horizon)):
        t[int(n):N, i] = 0.0; t[N + int(n):, i] = 0.0
    r = dict(res)
    r["traj"] = t
    return r


def oracle_loops_per_group(cfgname, sc, horizon, steps):
    """oracle_lib.rollout_chunk_full with {"N": n} per group of cars -> hist [steps, 9, B], status of every solve [steps, B]"""
    B = sc["state"].shape[1]
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    oh = np.zeros((steps, 9, B)); ost = np.zeros((steps, B), dtype=np.int32)
    for n in sorted(set(int(v) for v in horizon)):
        idx = np.nonzero(np.asarray(horizon) == n)[0]
        _, h, s = O.rollout_chunk_full((cfgname, {"N": n}, c(sc["state"][:, idx]), c(sc["coeffs"][:, idx]), c(sc["yaw_lo"][idx]), c(sc["yaw_hi"][idx]), steps))
        oh[:, :, idx] = h; ost[:, idx] = s
    return oh, ost


def twin_horizon_rollout(twin, params, sc, horizon, steps, opts, warm_start, model=None, weights=None):
    """Car by car through mpc::RolloutCar (the arguments of mpc_rollout_batch_device_fused_horizon)."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh = f(sc["state"]).copy(), f(sc["coeffs"]), f(sc["yaw_lo"]), f(sc["yaw_hi"])
    B = st.shape[1]
    md = f(model) if model is not None else None
    w = f(weights) if weights is not None else None
    hz = np.ascontiguousarray(horizon, dtype=np.int32)
    hist = np.zeros((steps, 9, B)); status = np.full(B, -99, dtype=np.int32); iters = np.full(B, -99, dtype=np.int32)
    sst = np.zeros((steps, B), dtype=np.int32); sit = np.zeros((steps, B), dtype=np.int32)
    rc = twin.mpc_horizon_twin_rollout(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(st), vp(cf), vp(yl), vp(yh), vp(w), vp(md),
                                       vp(hz), C.c_int(1 if warm_start else 0), C.byref(opts), vp(hist), vp(status), vp(iters), vp(sst), vp(sit))
    assert rc == 0, rc
    return {"hist": hist, "state": st, "status": status, "iters": iters, "step_status": sst, "step_iters": sit}


def twin_horizon_step_loop(twin, params, sc, horizon, steps, opts, warm_start):
    """Step by step: `steps` solves of the whole batch, the warm buffer and its status handed from one to the next."""
    B = sc["state"].shape[1]
    hist = np.zeros((steps, 9, B)); sst = np.zeros((steps, B), dtype=np.int32); sit = np.zeros((steps, B), dtype=np.int32)
    st = np.array(sc["state"], dtype=np.float64, copy=True)
    warm, wstat = None, None
    for k in range(steps):
        r = twin_horizon_solve(twin, params, dict(sc, state=st), horizon, opts, warm=warm if warm_start else None,
                               warm_status=wstat if warm_start else None, want_warm=True)
        hist[k] = r["out"]; sst[k] = r["status"]; sit[k] = r["iters"]
        st = r["out"][:6].copy(); warm, wstat = r["warm"], r["status"]
    return {"hist": hist, "state": st, "step_status": sst, "step_iters": sit}


def n_dt_study(pkg, golden_dir):
    """The 14 N / dt figures of the reference as ONE batch on an N = 50 config-stable.json handle (max_iter 3000): the entries, the
    handle's params, the batch (test.cpp's scenario in every column), weights [12, 14], model [6, 14] (dt from the entry, the rest
    the handle's) and horizon [14]."""
    from test_plot_anchors import _base_weights, _scenario
    a = load_golden("plot_anchors.json")
    cfg, pre, coef = _scenario()
    base = _base_weights(cfg, a)
    entries = list(a["n_dt"].items())
    B = len(entries)
    params = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"), N=50)
    params.max_iter = 3000
    model = pkg.scenarios.model_rows(params, B)
    model[0] = [r["dt"] for _, r in entries]
    horizon = np.array([r["N"] for _, r in entries], dtype=np.int32)
    sc = {"state": np.tile(np.array(list(pre.state))[:, None], (1, B)), "coeffs": np.tile(coef[:, None], (1, B)),
          "yaw_lo": np.full(B, pre.yaw_low), "yaw_hi": np.full(B, pre.yaw_high)}
    return entries, params, sc, np.tile(base[:, None], (1, B)).copy(), np.ascontiguousarray(model), horizon, pre


def judge_n_dt(entries, hist, worst, pre):
    """exactly as test_plot_anchors.test_twin_reproduces_every_n_dt_figure judges: <= 3 px, each entry's reproducible_samples, the
    30-01-2 episode"""
    from test_plot_anchors import PX_TOL, _px_dev
    for col, (name, r) in enumerate(entries):
        upto = r["reproducible_samples"]
        dev = _px_dev(r, hist, col, upto)
        assert max(dev.values()) <= PX_TOL, (name, dev)
        if upto == 26:
            assert worst[col] == 0, name
        if name == "30-01-2":
            assert np.all(np.abs(hist[21:, 6, col]) < 1e-6) and np.all(np.abs(hist[21:, 2, col] - pre.yaw_high) < 1e-6)
