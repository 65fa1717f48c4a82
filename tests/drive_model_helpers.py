"""Helpers of the tests of track driving with per-car model values (test infrastructure): the TEST-ONLY CPU build of the model loop
(tests/drive_model_twin), the plant as a composition of the oracle's Vehicle::move with every car's own Lf and max_steering, and the
oracle's telemetry handler with a per-car Config on recorded steps.  Shared by tests/test_drive_model.py and
tests/test_drive_model_gpu.py; tests/drive_helpers.py has everything that does not depend on the model array."""
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
from helpers import ROOT, TOL_STEER, vp
from run_model_helpers import car_config

_twin = None


def load_drive_model_twin():
    global _twin
    if _twin is None:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's own comes first, as in _abi.library)
        except ImportError:
            pass
        d = os.path.join(ROOT, "tests", "drive_model_twin")
        subprocess.check_call(["make", "-s", "-C", d])
        _twin = C.CDLL(os.path.join(d, "libdrive_model_twin.so"))
    return _twin


def twin_plant_model(twin, params, car, cmd, model, sub_old, sub_new, h):
    car, cmd, model = _f(car).copy(), _f(cmd), _f(model)
    B = car.shape[1]
    assert model.shape == (6, B)
    rc = twin.mpc_drive_model_twin_plant(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(cmd), vp(model), C.c_int(sub_old), C.c_int(sub_new),
                                         C.c_double(h))
    assert rc == 0, rc
    return car


def oracle_plant_model(cfgname, car, cmd, model, sub_old, sub_new, h):
    """drive_helpers.oracle_plant car by car, each with its own Config (Lf) and the reply scaled by its own max_steering"""
    out = np.array(car, dtype=np.float64, copy=True)
    for i in range(out.shape[1]):
        out[:, i:i + 1] = oracle_plant(car_config(cfgname, model, i), out[:, i:i + 1], cmd[:, i:i + 1], float(model[2, i]), sub_old, sub_new, h)
    return out


def twin_handler_model(twin, params, waypoints, car, k, model, opts, warm_opts, weights=None, warm=None, warm_status=None, want_warm=False):
    """One handler call of the CPU build on cars [6, B] with the windows that start at k and the columns of model -> cmd, status,
    iters, cte_epsi, warm."""
    tx, ty = track_of(waypoints)
    car, model = _f(car), _f(model)
    B = car.shape[1]
    k = np.ascontiguousarray(k, dtype=np.int32)
    rows = (params.N - 1) * 22
    cmd = np.zeros((2, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32); ce = np.zeros((2, B))
    wout = np.zeros((rows, B)) if (want_warm or warm is not None) else None
    warm = _f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_drive_model_twin_handler(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(k), vp(tx), vp(ty), C.c_int(len(tx)),
                                           vp(_f(weights)), vp(model), C.byref(opts), vp(warm), vp(warm_status), vp(wout), C.c_int64(B),
                                           C.byref(warm_opts), vp(cmd), vp(status), vp(iters), vp(ce))
    assert rc == 0, rc
    return {"cmd": cmd, "status": status, "iters": iters, "cte_epsi": ce, "warm": wout}


def twin_drive_model(twin, params, waypoints, car, model, steps, opts, warm_opts, weights=None):
    """mpc_drive_model_twin with the arguments of mpc_drive_batch_host_model -> car, summary, hist [steps, 13, B], status, iters."""
    tx, ty = track_of(waypoints)
    car, model = _f(car).copy(), _f(model)
    B = car.shape[1]
    assert model.shape == (6, B)
    summary = np.full((NSUM, B), SENTINEL); hist = np.full((steps, REC, B), SENTINEL)
    status = np.full(B, ISENTINEL, dtype=np.int32); iters = np.full(B, ISENTINEL, dtype=np.int32)
    rc = twin.mpc_drive_model_twin(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(car), vp(tx), vp(ty), C.c_int(len(tx)),
                                   vp(_f(weights)), vp(model), C.byref(opts), C.byref(warm_opts), vp(summary), vp(hist), vp(status), vp(iters))
    assert rc == 0, rc
    return {"car": car, "summary": summary, "hist": hist, "status": status, "iters": iters}


def oracle_check_steps_model(cfgname, over, model, waypoints, hist, extra):
    """On every recorded (car, window), the oracle's telemetry handler with the car's own Config: the same status, the steer within
    TOL_STEER taken in radians of the car's own max_steering, the throttle within TOL_THROTTLE.  No (car, step) pair is left out.
    -> (max |d steer| [rad], max |d throttle|, pairs compared)."""
    steps, _, B = hist.shape
    d_steer = d_thr = 0.0
    pairs = 0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in range(B):
            cfg = car_config(cfgname, model, i, **over)          # (a fresh one per call: run() mutates the yaw bounds of its Config)
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], extra)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            assert st == 0, (t, i, st)                           # the stated population: every solve ends SUCCESS in the oracle
            d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * float(model[2, i]))
            d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
            pairs += 1
    assert pairs == steps * B
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr, pairs


# ---- the device side (tests/test_drive_model_gpu.py) ------------------------------------------------------------------------------
CHILD_TIMEOUT_S = 120


def to_device(a, dev, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def fast_params(pkg, golden_dir, **over):
    return pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), **dict(dict(N=10), **over))


def device_drive(pkg, params, waypoints, car, model, steps, dev, warm=0, weights=None, hist=True, pad=3, host=False, fused=False, plain=False):
    """The _model entry points through the raw ABI with ld = B + pad (plain: the entry points without _model, and no model argument;
    model None otherwise: model = NULL).  Inputs hold NaN from column B on, outputs the sentinels everywhere before the call.  -> the
    arrays cut to B, after checking that nothing behind column B was written; and the handle's mpc_drive_info."""
    import torch
    lib = pkg.library()
    B = car.shape[1]
    ld = B + pad
    tx, ty = track_of(waypoints)
    opts = pkg.drive_opts_default(params, warm_start=warm)

    def wide(a, fill=np.nan):
        w = np.full((a.shape[0], ld), fill); w[:, :B] = a
        return w
    h_car = wide(car); h_w = wide(weights) if weights is not None else None; h_m = wide(model) if model is not None else None
    h_sum = np.full((NSUM, ld), SENTINEL); h_hist = np.full((steps, REC, ld), SENTINEL) if hist else None
    h_st = np.full(ld, ISENTINEL, dtype=np.int32); h_it = np.full(ld, ISENTINEL, dtype=np.int32)
    name = "mpc_drive_batch_host" if host else ("mpc_drive_batch_device_fused" if fused else "mpc_drive_batch_device")
    call = getattr(lib, name if plain else name + "_model")
    with pkg.BatchedMPC(params, max(B, 1), device=0) as mpc:
        if host:
            p = lambda a: a.ctypes.data if a is not None else None
            m = () if plain else (p(h_m),)
            rc = call(mpc._h, B, ld, steps, p(h_car), p(tx), p(ty), len(tx), p(h_w), *m, C.byref(opts), None, p(h_sum), p(h_hist), p(h_st), p(h_it))
            assert rc == 0, lib.mpc_last_error()
            got = {"car": h_car, "summary": h_sum, "hist": h_hist, "status": h_st, "iters": h_it}
        else:
            d = {"car": to_device(h_car, dev), "summary": to_device(h_sum, dev), "hist": to_device(h_hist, dev) if hist else None, "status": to_device(h_st, dev, np.int32),
                 "iters": to_device(h_it, dev, np.int32)}
            d_tx, d_ty, d_w = to_device(tx, dev), to_device(ty, dev), to_device(h_w, dev) if h_w is not None else None
            d_m = to_device(h_m, dev) if h_m is not None else None
            p = lambda t: t.data_ptr() if t is not None else None
            m = () if plain else (p(d_m),)
            rc = call(mpc._h, B, ld, steps, p(d["car"]), p(d_tx), p(d_ty), len(tx), p(d_w), *m, C.byref(opts), None, p(d["summary"]), p(d["hist"]),
                      p(d["status"]), p(d["iters"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert rc == 0, lib.mpc_last_error()
            torch.cuda.synchronize()
            got = {k: (v.cpu().numpy() if v is not None else None) for k, v in d.items()}
        info = mpc.drive_info()
    assert np.isnan(got["car"][:, B:]).all() and (got["summary"][:, B:] == SENTINEL).all() and (got["status"][B:] == ISENTINEL).all() and (got["iters"][B:] == ISENTINEL).all()
    if hist:
        assert (got["hist"][:, :, B:] == SENTINEL).all()
    out = {k: (v[..., :B].copy() if v is not None else None) for k, v in got.items()}
    assert (out["summary"] != SENTINEL).all() and (out["status"] != ISENTINEL).all() and (out["iters"] != ISENTINEL).all()
    out["info"] = info
    return out


def containment_case(pkg, params, waypoints):
    """80 cars with the columns draw_rows(seed 9), clean and dirty -> car, model, dirty car, dirty model, the cars that must end
    INFEASIBLE at every step (an unusable column: NaN, dt = 0; a car at twice its own top speed), all cars that carry a status."""
    from model_helpers import draw_rows
    car = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    model = draw_rows(params, 80, seed=9)
    d_car, d_model = car.copy(), model.copy()
    d_model[2, 3] = np.nan; d_model[0, 21] = 0.0
    d_model[5, 40] = 0.5 * car[3, 40] * 1609.34 / 3600.0          # its own top speed: half of what it is driving
    d_car[0, 5] = np.nan; d_car[0, 70] += 1e6
    return car, model, d_car, d_model, [3, 21, 40], [3, 21, 40, 5, 70]


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
    car, model, d_car, d_model, _, _ = containment_case(pkg, params, wp)
    dev = torch.device("cuda:0")
    out = {}
    for warm in (0, 1):
        for tag, c, m in (("clean", car, model), ("dirty", d_car, d_model)):
            r = device_drive(pkg, params, wp, c, m, 4, dev, warm=warm, fused=spec["fused"])
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
