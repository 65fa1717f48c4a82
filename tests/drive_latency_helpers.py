"""Helpers of the tests of track driving with per-car latency (test infrastructure): the TEST-ONLY CPU build of the latency loop
(tests/drive_latency_twin), the drawn columns, the plant as a composition of the oracle's Vehicle::move with every car's own substep
counts, and the oracle's telemetry handler with a per-car Config (latency, lookahead) on recorded steps.  Shared by
tests/test_drive_latency.py and tests/test_drive_latency_gpu.py; tests/drive_helpers.py and tests/drive_model_helpers.py have
everything that does not depend on the latency array."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import oracle_lib as O
from drive_helpers import (ISENTINEL, NSUM, REC, REC_CMD, REC_K, REC_STATUS, SENTINEL, TOL_THROTTLE, _f, oracle_plant, track_of,
                           window_points)
from drive_model_helpers import fast_params, to_device
from helpers import ROOT, TOL_STEER, vp

COMP, SUB_OLD, SUB_NEW = 0, 1, 2
_twin = None


def load_drive_latency_twin():
    global _twin
    if _twin is None:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's own comes first, as in _abi.library)
        except ImportError:
            pass
        d = os.path.join(ROOT, "tests", "drive_latency_twin")
        subprocess.check_call(["make", "-s", "-C", d])
        _twin = C.CDLL(os.path.join(d, "libdrive_latency_twin.so"))
    return _twin


def draw_latency(B, seed=21):
    """The stated population, drawn in this order with default_rng(seed): comp uniform in [0, 0.25] s, then about a quarter of the cars
    (uniform < 0.25) set to exactly 0; sub_old an integer in 0..25; sub_new an integer in 1..12.  Final ranges: the stated ones, not narrowed; final seed: 21.  On
    the 16 cars x 8 messages of tests/test_drive_latency.py (config-fast and config-stable, cold and warm) the oracle alone ends every
    recorded solve SUCCESS with them, so no (car, step) pair is left out of a comparison."""
    g = np.random.default_rng(seed)
    comp = g.uniform(0.0, 0.25, B)
    comp[g.uniform(0.0, 1.0, B) < 0.25] = 0.0
    return np.ascontiguousarray(np.stack([comp, g.integers(0, 26, B).astype(np.float64), g.integers(1, 13, B).astype(np.float64)]))


def uniform_latency(B, comp, sub_old, sub_new):
    return np.ascontiguousarray(np.repeat(np.array([[float(comp)], [float(sub_old)], [float(sub_new)]]), B, axis=1))


def handle_comp(params, extra=0.0):
    """what a handle's own rule compensates for: lookahead + extra_latency, or 0 on a handle with latency_ms = 0"""
    return params.lookahead + extra if params.latency_ms != 0 else 0.0


def twin_plant_latency(twin, params, car, cmd, model, latency, opts):
    car, cmd, model, latency = _f(car).copy(), _f(cmd), _f(model), _f(latency)
    B = car.shape[1]
    assert model.shape == (6, B) and latency.shape == (3, B)
    rc = twin.mpc_drive_latency_twin_plant(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(cmd), vp(model), vp(latency), C.byref(opts))
    assert rc == 0, rc
    return car


def oracle_plant_latency(cfgname, car, cmd, max_steering, latency, h):
    """drive_helpers.oracle_plant car by car, each with its own substep counts"""
    out = np.array(car, dtype=np.float64, copy=True)
    cfg = O.load_config(cfgname)
    for i in range(out.shape[1]):
        out[:, i:i + 1] = oracle_plant(cfg, out[:, i:i + 1], cmd[:, i:i + 1], max_steering, int(latency[SUB_OLD, i]), int(latency[SUB_NEW, i]), h)
    return out


def twin_handler_latency(twin, params, waypoints, car, comp, k, model, opts, warm_opts, weights=None, warm=None, warm_status=None, want_warm=False):
    """One handler call of the CPU build on cars [6, B] with the windows that start at k, compensating comp [B] -> cmd, status, iters,
    cte_epsi, warm."""
    tx, ty = track_of(waypoints)
    car, model, comp = _f(car), _f(model), _f(comp)
    B = car.shape[1]
    k = np.ascontiguousarray(k, dtype=np.int32)
    rows = (params.N - 1) * 22
    cmd = np.zeros((2, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32); ce = np.zeros((2, B))
    wout = np.zeros((rows, B)) if (want_warm or warm is not None) else None
    warm = _f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_drive_latency_twin_handler(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(comp), vp(k), vp(tx), vp(ty), C.c_int(len(tx)),
                                             vp(_f(weights)), vp(model), C.byref(opts), vp(warm), vp(warm_status), vp(wout), C.c_int64(B),
                                             C.byref(warm_opts), vp(cmd), vp(status), vp(iters), vp(ce))
    assert rc == 0, rc
    return {"cmd": cmd, "status": status, "iters": iters, "cte_epsi": ce, "warm": wout}


def twin_drive_latency(twin, params, waypoints, car, model, latency, steps, opts, warm_opts, weights=None):
    """mpc_drive_latency_twin with the arguments of mpc_drive_batch_host_latency -> car, summary, hist [steps, 13, B], status, iters."""
    tx, ty = track_of(waypoints)
    car, model, latency = _f(car).copy(), _f(model), _f(latency)
    B = car.shape[1]
    assert model.shape == (6, B) and latency.shape == (3, B)
    summary = np.full((NSUM, B), SENTINEL); hist = np.full((steps, REC, B), SENTINEL)
    status = np.full(B, ISENTINEL, dtype=np.int32); iters = np.full(B, ISENTINEL, dtype=np.int32)
    rc = twin.mpc_drive_latency_twin(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(car), vp(tx), vp(ty), C.c_int(len(tx)),
                                     vp(_f(weights)), vp(model), vp(latency), C.byref(opts), C.byref(warm_opts), vp(summary), vp(hist), vp(status),
                                     vp(iters))
    assert rc == 0, rc
    return {"car": car, "summary": summary, "hist": hist, "status": status, "iters": iters}


def oracle_check_steps_latency(cfgname, over, params, latency, waypoints, hist):
    """On every recorded (car, window), the oracle's telemetry handler with the car's own Config -- latency = 1 if comp > 0 else 0,
    lookahead = comp -- and extra = 0: the same status, the steer within TOL_STEER (radians), the throttle within TOL_THROTTLE.  No
    (car, step) pair is left out.  -> (max |d steer| [rad], max |d throttle|, pairs compared)."""
    steps, _, B = hist.shape
    d_steer = d_thr = 0.0
    pairs = 0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in range(B):
            comp = float(latency[COMP, i])
            cfg = O.load_config(cfgname, **dict(over, latency=1 if comp > 0 else 0, lookahead=comp))     # (a fresh one per call: run() mutates it)
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], 0.0)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            assert st == 0, (t, i, st)                           # the stated population: every solve ends SUCCESS in the oracle
            d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * params.max_steering)
            d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
            pairs += 1
    assert pairs == steps * B
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr, pairs


def unusable(latency, cars):
    """The four unusable columns of the issue in the cars `cars` (4 of them) of a copy: NaN, comp = -1, sub_old = 2.5,
    sub_old + sub_new = 1001."""
    d = np.array(latency, dtype=np.float64, copy=True)
    a, b, c, e = cars
    d[COMP, a] = np.nan
    d[COMP, b] = -1.0
    d[SUB_OLD, c] = 2.5
    d[SUB_OLD, e] = 1001.0 - d[SUB_NEW, e]
    return d


# ---- the device side (tests/test_drive_latency_gpu.py) ----------------------------------------------------------------------------
CHILD_TIMEOUT_S = 120
FORMS = {"device": "mpc_drive_batch_device", "fused": "mpc_drive_batch_device_fused", "host": "mpc_drive_batch_host"}


def device_drive(pkg, params, waypoints, car, steps, dev, model=None, latency=None, form="device", entry="latency", warm=0, weights=None, hist=True,
                 pad=3, opts_over=None, mpc=None):
    """A drive entry point through the raw ABI with ld = B + pad.  entry: "latency" (model and latency may be None: NULL), "model"
    (no latency argument), "plain" (neither).  Inputs hold NaN from column B on, outputs the sentinels everywhere before the call.  ->
    the arrays cut to B, after checking that nothing behind column B was written; and the handle's mpc_drive_info.  mpc: a live
    handle to use (its info then counts every call made on it)."""
    import torch
    lib = pkg.library()
    B = car.shape[1]
    ld = B + pad
    tx, ty = track_of(waypoints)
    opts = pkg.drive_opts_default(params, warm_start=warm, **(opts_over or {}))

    def wide(a, fill=np.nan):
        if a is None:
            return None
        w = np.full((a.shape[0], ld), fill); w[:, :B] = a
        return w
    h_car, h_w, h_m, h_l = wide(car), wide(weights), wide(model), wide(latency)
    h_sum = np.full((NSUM, ld), SENTINEL); h_hist = np.full((steps, REC, ld), SENTINEL) if hist else None
    h_st = np.full(ld, ISENTINEL, dtype=np.int32); h_it = np.full(ld, ISENTINEL, dtype=np.int32)
    host = form == "host"
    call = getattr(lib, FORMS[form] + {"latency": "_latency", "model": "_model", "plain": ""}[entry])
    own = mpc is None
    if own:
        mpc = pkg.BatchedMPC(params, max(B, 1), device=0)
    try:
        if host:
            p = lambda a: a.ctypes.data if a is not None else None
            ex = {"latency": (p(h_m), p(h_l)), "model": (p(h_m),), "plain": ()}[entry]
            rc = call(mpc._h, B, ld, steps, p(h_car), p(tx), p(ty), len(tx), p(h_w), *ex, C.byref(opts), None, p(h_sum), p(h_hist), p(h_st), p(h_it))
            assert rc == 0, lib.mpc_last_error()
            got = {"car": h_car, "summary": h_sum, "hist": h_hist, "status": h_st, "iters": h_it}
        else:
            dd = lambda a, dt=np.float64: to_device(a, dev, dt) if a is not None else None
            d = {"car": dd(h_car), "summary": dd(h_sum), "hist": dd(h_hist), "status": dd(h_st, np.int32), "iters": dd(h_it, np.int32)}
            d_tx, d_ty, d_w, d_m, d_l = dd(tx), dd(ty), dd(h_w), dd(h_m), dd(h_l)
            p = lambda t: t.data_ptr() if t is not None else None
            ex = {"latency": (p(d_m), p(d_l)), "model": (p(d_m),), "plain": ()}[entry]
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


KEYS = ("car", "summary", "hist", "status", "iters")


def same(a, b, keys=KEYS, cars=None):
    """bitwise, NaN == NaN included (a contained car may hold one in both)"""
    for k in keys:
        if a[k] is None or b[k] is None:      # (a call without hist: everything else is compared)
            continue
        x, y = (a[k], b[k]) if cars is None else (a[k][..., cars], b[k][..., cars])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


BAD_COLUMNS = [3, 21, 40, 55]          # the cars of containment_case with an unusable column
BAD_CARS = [5, 70]                     # ... and those no caller should send: x = NaN, 1e6 m off the track


def containment_case(pkg, params, waypoints):
    """80 cars with the columns draw_latency(80, seed 22), clean and dirty -> car, latency, dirty car, dirty latency."""
    car = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    latency = draw_latency(80, seed=22)
    d_car, d_lat = car.copy(), unusable(latency, BAD_COLUMNS)
    d_car[0, 5] = np.nan; d_car[0, 70] += 1e6
    return car, latency, d_car, d_lat


def child_main(path):
    """Runs in the child: the clean and the dirty batch of containment_case on the device, cold and warm, results into an .npz."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    import torch
    pkg = G.load_package()
    spec = json.load(open(path + ".json"))
    gd = os.path.join(ROOT, "tests", "golden")
    params = fast_params(pkg, gd, wave_max_batch=spec["wave_max_batch"])
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    car, lat, d_car, d_lat = containment_case(pkg, params, wp)
    dev = torch.device("cuda:0")
    out = {}
    for warm in (0, 1):
        for tag, c, l in (("clean", car, lat), ("dirty", d_car, d_lat)):
            r = device_drive(pkg, params, wp, c, 4, dev, latency=l, warm=warm, form="fused" if spec["fused"] else "device")
            for k in ("car", "summary", "hist", "status", "iters"):
                out["%d/%s/%s" % (warm, tag, k)] = r[k]
            out["%d/%s/info" % (warm, tag)] = np.array([r["info"]["fused_launches"], r["info"]["stepwise_loops"]])
    np.savez(path, **out)


def run_containment_in_child(wave_max_batch, fused, timeout=CHILD_TIMEOUT_S):
    """-> {(warm, "clean" | "dirty"): the arrays of device_drive}; a child that does not end within `timeout` seconds fails the caller
    (subprocess.TimeoutExpired) after it has been killed"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "containment.npz")
        json.dump({"wave_max_batch": int(wave_max_batch), "fused": bool(fused)}, open(path + ".json", "w"))
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
