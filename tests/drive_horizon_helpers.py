"""Helpers of the tests of track driving with a per-car horizon (test infrastructure): the TEST-ONLY CPU build of the horizon loop
(tests/drive_horizon_twin), the oracle's telemetry handler with N = horizon[i] on recorded steps, the unusable horizons, and the device
side through the raw ABI.  Shared by tests/test_drive_horizon.py and tests/test_drive_horizon_gpu.py; tests/drive_helpers.py,
tests/drive_model_helpers.py and tests/drive_latency_helpers.py have everything that does not depend on the horizon array."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import oracle_lib as O
from drive_helpers import (ISENTINEL, NSUM, REC, REC_CMD, REC_K, REC_STATUS, SENTINEL, TOL_THROTTLE, _f, track_of, window_points)
from drive_latency_helpers import KEYS, draw_latency, handle_comp, same, uniform_latency      # noqa: F401  (re-exported)
from drive_model_helpers import fast_params, to_device
from helpers import ROOT, TOL_STEER, vp
from horizon_helpers import LOOP_HORIZONS

INFEASIBLE = 3
_twin = None


def load_drive_horizon_twin():
    global _twin
    if _twin is None:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's own comes first, as in _abi.library)
        except ImportError:
            pass
        d = os.path.join(ROOT, "tests", "drive_horizon_twin")
        subprocess.check_call(["make", "-s", "-C", d])
        _twin = C.CDLL(os.path.join(d, "libdrive_horizon_twin.so"))
    return _twin


def _hz(horizon):
    return np.ascontiguousarray(horizon, dtype=np.int32)


def mixed_horizons(B, choices=LOOP_HORIZONS):
    """choices[i % len(choices)]"""
    return _hz([choices[i % len(choices)] for i in range(B)])


def default_latency(params, opts, B):
    """the columns that say what the call's own scalars say (the twin always takes a latency array)"""
    return uniform_latency(B, handle_comp(params, opts.extra_latency), opts.sub_old, opts.sub_new)


def twin_drive_horizon(twin, params, waypoints, car, horizon, steps, opts, warm_opts, model=None, latency=None, weights=None):
    """mpc_drive_horizon_twin with the arguments of mpc_drive_batch_host_horizon -> car, summary, hist [steps, 13, B], status, iters.
    latency None: the columns of the call's own scalars."""
    tx, ty = track_of(waypoints)
    car, model, horizon = _f(car).copy(), _f(model), _hz(horizon)
    B = car.shape[1]
    latency = _f(latency) if latency is not None else default_latency(params, opts, B)
    assert (model is None or model.shape == (6, B)) and latency.shape == (3, B) and horizon.shape == (B,)
    summary = np.full((NSUM, B), SENTINEL); hist = np.full((steps, REC, B), SENTINEL)
    status = np.full(B, ISENTINEL, dtype=np.int32); iters = np.full(B, ISENTINEL, dtype=np.int32)
    rc = twin.mpc_drive_horizon_twin(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(car), vp(tx), vp(ty), C.c_int(len(tx)),
                                     vp(_f(weights)), vp(model), vp(horizon), vp(latency), C.byref(opts), C.byref(warm_opts), vp(summary), vp(hist),
                                     vp(status), vp(iters))
    assert rc == 0, rc
    return {"car": car, "summary": summary, "hist": hist, "status": status, "iters": iters}


def twin_handler_horizon(twin, params, waypoints, car, comp, k, horizon, opts, warm_opts, model=None, weights=None, warm=None, warm_status=None,
                         want_warm=False):
    """One handler call of the CPU build on cars [6, B] with the windows that start at k, compensating comp [B], horizon [B] -> cmd,
    status, iters, cte_epsi, warm (the rows of params.N)."""
    tx, ty = track_of(waypoints)
    car, model, comp, horizon = _f(car), _f(model), _f(comp), _hz(horizon)
    B = car.shape[1]
    k = np.ascontiguousarray(k, dtype=np.int32)
    rows = (params.N - 1) * 22
    cmd = np.zeros((2, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32); ce = np.zeros((2, B))
    wout = (np.array(warm, dtype=np.float64, copy=True) if warm is not None else np.zeros((rows, B))) if (want_warm or warm is not None) else None
    warm = _f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_drive_horizon_twin_handler(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(comp), vp(k), vp(tx), vp(ty), C.c_int(len(tx)),
                                             vp(_f(weights)), vp(model), vp(horizon), C.byref(opts), vp(warm), vp(warm_status), vp(wout), C.c_int64(B),
                                             C.byref(warm_opts), vp(cmd), vp(status), vp(iters), vp(ce))
    assert rc == 0, rc
    return {"cmd": cmd, "status": status, "iters": iters, "cte_epsi": ce, "warm": wout}


def oracle_check_steps_horizon(cfgname, params, horizon, waypoints, hist, extra=0.0):
    """On every recorded (car, window), the oracle's telemetry handler on a config loaded with N = horizon[i]: the same status, the steer
    within TOL_STEER / max_steering and the throttle within TOL_THROTTLE (the bounds of drive_helpers.oracle_check_steps).  No (car,
    step) pair is left out.  -> (max |d steer| [rad], max |d throttle|, pairs compared)."""
    steps, _, B = hist.shape
    d_steer = d_thr = 0.0
    pairs = 0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in range(B):
            cfg = O.load_config(cfgname, N=int(horizon[i]))          # (a fresh one per call: run() mutates it)
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], extra)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            assert st == 0, (t, i, st)                                # the stated inputs: every solve ends SUCCESS
            d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * params.max_steering)
            d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
            pairs += 1
    assert pairs == steps * B
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr, pairs


def unusable(horizon, cars, N):
    """The four unusable horizons of the issue -- 2, 0, -1, N + 1 -- in the cars `cars` (4 of them) of a copy."""
    d = _hz(horizon).copy()
    d[list(cars)] = [2, 0, -1, N + 1]
    return d


def check_unusable(res, clean, bad, steps):
    """those cars INFEASIBLE at every step, summary row 7 = steps, no not-a-number; every other car bitwise the clean batch"""
    assert (res["hist"][:, REC_STATUS][:, bad] == INFEASIBLE).all() and (res["status"][bad] == INFEASIBLE).all()
    assert (res["summary"][7, bad] == steps).all()
    for k in ("car", "summary", "hist"):
        assert np.isfinite(res[k][..., bad]).all(), k
    good = np.setdiff1d(np.arange(res["status"].shape[0]), bad)
    same(res, clean, cars=good)


# ---- the device side (tests/test_drive_horizon_gpu.py) ----------------------------------------------------------------------------
CHILD_TIMEOUT_S = 120
FORMS = {"device": "mpc_drive_batch_device", "fused": "mpc_drive_batch_device_fused", "host": "mpc_drive_batch_host"}
HZ_PAD = -999          # what the horizon array holds from column B on


def device_drive(pkg, params, waypoints, car, steps, dev, horizon=None, model=None, latency=None, form="device", entry="horizon", warm=0, weights=None,
                 hist=True, pad=3, opts_over=None, mpc=None):
    """A drive entry point through the raw ABI with ld = B + pad.  entry: "horizon" (model, horizon and latency may each be None: NULL)
    or "latency" (no horizon argument).  Inputs hold NaN (the horizons: HZ_PAD) from column B on, outputs the sentinels everywhere
    before the call.  -> the arrays cut to B, after checking that nothing behind column B was written; and the handle's mpc_drive_info.
    mpc: a live handle to use (its info then counts every call made on it)."""
    import torch
    lib = pkg.library()
    B = car.shape[1]
    ld = B + pad
    tx, ty = track_of(waypoints)
    opts = pkg.drive_opts_default(params, warm_start=warm, **(opts_over or {}))
    assert entry in ("horizon", "latency") and (entry == "horizon" or horizon is None)

    def wide(a, fill=np.nan):
        if a is None:
            return None
        w = np.full((a.shape[0], ld), fill); w[:, :B] = a
        return w
    h_car, h_w, h_m, h_l = wide(car), wide(weights), wide(model), wide(latency)
    h_hz = None
    if horizon is not None:
        h_hz = np.full(ld, HZ_PAD, dtype=np.int32); h_hz[:B] = horizon
    h_sum = np.full((NSUM, ld), SENTINEL); h_hist = np.full((steps, REC, ld), SENTINEL) if hist else None
    h_st = np.full(ld, ISENTINEL, dtype=np.int32); h_it = np.full(ld, ISENTINEL, dtype=np.int32)
    host = form == "host"
    call = getattr(lib, FORMS[form] + "_" + entry)
    own = mpc is None
    if own:
        mpc = pkg.BatchedMPC(params, max(B, 1), device=0)
    try:
        if host:
            p = lambda a: a.ctypes.data if a is not None else None
            ex = (p(h_m), p(h_hz), p(h_l)) if entry == "horizon" else (p(h_m), p(h_l))
            rc = call(mpc._h, B, ld, steps, p(h_car), p(tx), p(ty), len(tx), p(h_w), *ex, C.byref(opts), None, p(h_sum), p(h_hist), p(h_st), p(h_it))
            assert rc == 0, lib.mpc_last_error()
            got = {"car": h_car, "summary": h_sum, "hist": h_hist, "status": h_st, "iters": h_it}
        else:
            dd = lambda a, dt=np.float64: to_device(a, dev, dt) if a is not None else None
            d = {"car": dd(h_car), "summary": dd(h_sum), "hist": dd(h_hist), "status": dd(h_st, np.int32), "iters": dd(h_it, np.int32)}
            d_tx, d_ty, d_w, d_m, d_l, d_hz = dd(tx), dd(ty), dd(h_w), dd(h_m), dd(h_l), dd(h_hz, np.int32)
            p = lambda t: t.data_ptr() if t is not None else None
            ex = (p(d_m), p(d_hz), p(d_l)) if entry == "horizon" else (p(d_m), p(d_l))
            rc = call(mpc._h, B, ld, steps, p(d["car"]), p(d_tx), p(d_ty), len(tx), p(d_w), *ex, C.byref(opts), None, p(d["summary"]), p(d["hist"]),
                      p(d["status"]), p(d["iters"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert rc == 0, lib.mpc_last_error()
            torch.cuda.synchronize()
            got = {k: (v.cpu().numpy() if v is not None else None) for k, v in d.items()}
        info = mpc.drive_info()
    finally:
        if own:
            mpc.close()
    assert np.isnan(got["car"][:, B:]).all() and (got["summary"][:, B:] == SENTINEL).all() and (got["status"][B:] == ISENTINEL).all() and (got["iters"][B:] == ISENTINEL).all()
    if hist:
        assert (got["hist"][:, :, B:] == SENTINEL).all()
    out = {k: (v[..., :B].copy() if v is not None else None) for k, v in got.items()}
    assert (out["summary"] != SENTINEL).all() and (out["status"] != ISENTINEL).all() and (out["iters"] != ISENTINEL).all()
    out["info"] = info
    return out


BAD_HORIZONS = [3, 21, 40, 55]         # the cars of containment_case with an unusable horizon (2, 0, -1, N + 1)
BAD_CARS = [5, 70]                     # ... and those no caller should send: x = NaN, 1e6 m off the track


def containment_case(pkg, params, waypoints):
    """80 cars with the horizons LOOP_HORIZONS[i % 5], clean and dirty -> car, horizon, dirty car, dirty horizon."""
    car = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    hz = mixed_horizons(80)
    d_car, d_hz = car.copy(), unusable(hz, BAD_HORIZONS, params.N)
    d_car[0, 5] = np.nan; d_car[0, 70] += 1e6
    return car, hz, d_car, d_hz


def child_main(path):
    """Runs in the child: the clean and the dirty batch of containment_case on the device, cold and warm, results into an .npz.  Every
    drive is one call; nothing is retried."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    import torch
    pkg = G.load_package()
    spec = json.load(open(path + ".json"))
    gd = os.path.join(ROOT, "tests", "golden")
    params = fast_params(pkg, gd)
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    car, hz, d_car, d_hz = containment_case(pkg, params, wp)
    dev = torch.device("cuda:0")
    out = {}
    for warm in (0, 1):
        for tag, c, n in (("clean", car, hz), ("dirty", d_car, d_hz)):
            r = device_drive(pkg, params, wp, c, 4, dev, horizon=n, warm=warm, form="fused" if spec["fused"] else "device")
            for k in KEYS:
                out["%d/%s/%s" % (warm, tag, k)] = r[k]
            out["%d/%s/info" % (warm, tag)] = np.array([r["info"]["fused_launches"], r["info"]["stepwise_loops"]])
    np.savez(path, **out)


def run_containment_in_child(fused, timeout=CHILD_TIMEOUT_S):
    """-> {(warm, "clean" | "dirty"): the arrays of device_drive}; a child that does not end within `timeout` seconds fails the caller
    (subprocess.TimeoutExpired) after it has been killed; the parent checks the exit status"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "containment.npz")
        json.dump({"fused": bool(fused)}, open(path + ".json", "w"))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=timeout, env=env)
        assert p.returncode == 0, p.stderr[-4000:]
        z = np.load(path)
        res = {}
        for key in z.files:
            warm, tag, k = key.split("/")
            res.setdefault((int(warm), tag), {})[k] = z[key]
        for r in res.values():
            r["info"] = {"fused_launches": int(r["info"][0]), "stepwise_loops": int(r["info"][1])}
    return res


if __name__ == "__main__":
    child_main(sys.argv[1])
