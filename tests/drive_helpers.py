"""Helpers of the track-driving tests (test infrastructure): the TEST-ONLY CPU build of the drive loop (tests/drive_twin), numpy's
statement of the summary rows, the plant as a composition of the oracle's Vehicle::move, and the oracle's telemetry handler on
recorded steps -- the comparison is solve by solve, so loop amplification cannot enter.  Shared by tests/test_drive.py and
tests/test_drive_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
from helpers import ROOT, TOL_STEER, vp

NSUM, REC = 8, 13
REC_CMD, REC_CTE, REC_EPSI, REC_STATUS, REC_ITERS, REC_K = 6, 8, 9, 10, 11, 12
TOL_THROTTLE = 1e-5        # the bound tests/test_run_warm_gpu.py uses for the handler's throttle
SENTINEL, ISENTINEL = -7777.25, -12345

_twin = None


def load_drive_twin():
    global _twin
    if _twin is None:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's own comes first, as in _abi.library)
        except ImportError:
            pass
        d = os.path.join(ROOT, "tests", "drive_twin")
        subprocess.check_call(["make", "-s", "-C", d])
        _twin = C.CDLL(os.path.join(d, "libdrive_twin.so"))
    return _twin


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64) if a is not None else None


def track_of(waypoints):
    wp = np.asarray(waypoints, dtype=np.float64)
    return np.ascontiguousarray(wp[:, 0]), np.ascontiguousarray(wp[:, 1])


def twin_window(twin, waypoints, x, y):
    tx, ty = track_of(waypoints)
    x, y = _f(x), _f(y)
    k = np.full(len(x), ISENTINEL, dtype=np.int32)
    assert twin.mpc_drive_twin_window(vp(tx), vp(ty), C.c_int(len(tx)), C.c_int64(len(x)), vp(x), vp(y), vp(k)) == 0
    return k


def window_points(waypoints, k, npts=6):
    """w[k .. k + npts - 1], cyclically -> ptsx, ptsy [npts, B]"""
    wp = np.asarray(waypoints, dtype=np.float64)
    idx = (np.asarray(k, dtype=np.int64)[None, :] + np.arange(npts)[:, None]) % len(wp)
    return np.ascontiguousarray(wp[idx, 0]), np.ascontiguousarray(wp[idx, 1])


def twin_plant(twin, params, car, cmd, sub_old, sub_new, h):
    car, cmd = _f(car).copy(), _f(cmd)
    B = car.shape[1]
    assert twin.mpc_drive_twin_plant(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(cmd), C.c_int(sub_old), C.c_int(sub_new), C.c_double(h)) == 0
    return car


def oracle_plant(cfg, car, cmd, max_steering, sub_old, sub_new, h):
    """The plant as the issue states it, one car at a time: substeps of the oracle's Vehicle::move (O.vehicle_move) under the handler's
    reading of the car -- v = mph2mps(speed), steer = -steering_angle, accel = (throttle - v / 50) * 6 --, the reply taking effect after
    sub_old of them unless it is not finite."""
    out = np.array(car, dtype=np.float64, copy=True)
    for i in range(out.shape[1]):
        c = out[:, i].copy()

        def sub():
            v = c[3] * 1609.34 / 3600.0
            p = O.vehicle_move(cfg, [c[0], c[1], c[2], v, -c[4], (c[5] - v / 50.0) * 6.0], h)
            c[0], c[1], c[2], c[3] = p[0], p[1], p[2], p[3] * 3600.0 / 1609.34
        for _ in range(sub_old):
            sub()
        if np.isfinite(cmd[0, i]) and np.isfinite(cmd[1, i]):
            c[4], c[5] = cmd[0, i] * max_steering, cmd[1, i]
        for _ in range(sub_new):
            sub()
        out[:, i] = c
    return out


def numpy_plant(car, cmd, params, sub_old, sub_new, h):
    """The plant for a whole batch in numpy (the loop a caller writes without the drive entry points; tools/drive_bench.py): the
    substeps of oracle_plant, vectorised.  -> the next cars [6, B]."""
    def sub(c):
        v = c[3] * 1609.34 / 3600.0
        dist = v * h
        acc = (c[5] - v / 50.0) * 6.0
        return np.stack([c[0] + dist * np.cos(c[2]), c[1] + dist * np.sin(c[2]), c[2] - c[4] * dist / params.Lf, (v + acc * h) * 3600.0 / 1609.34, c[4], c[5]])
    car = np.array(car, dtype=np.float64, copy=True)
    for _ in range(sub_old):
        car = sub(car)
    ok = np.isfinite(cmd[0]) & np.isfinite(cmd[1])
    car[4] = np.where(ok, cmd[0] * params.max_steering, car[4]); car[5] = np.where(ok, cmd[1], car[5])
    for _ in range(sub_new):
        car = sub(car)
    return np.ascontiguousarray(car)


def twin_handler(twin, params, waypoints, car, k, opts, warm_opts, weights=None, warm=None, warm_status=None, want_warm=False):
    """One handler call of the CPU build on cars [6, B] with the windows that start at k -> cmd, status, iters, cte_epsi, warm."""
    tx, ty = track_of(waypoints)
    car = _f(car)
    B = car.shape[1]
    k = np.ascontiguousarray(k, dtype=np.int32)
    rows = (params.N - 1) * 22
    cmd = np.zeros((2, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32); ce = np.zeros((2, B))
    wout = np.zeros((rows, B)) if (want_warm or warm is not None) else None
    warm = _f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_drive_twin_handler(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(k), vp(tx), vp(ty), C.c_int(len(tx)), vp(_f(weights)),
                                     C.byref(opts), vp(warm), vp(warm_status), vp(wout), C.c_int64(B), C.byref(warm_opts), vp(cmd), vp(status),
                                     vp(iters), vp(ce))
    assert rc == 0, rc
    return {"cmd": cmd, "status": status, "iters": iters, "cte_epsi": ce, "warm": wout}


def twin_drive(twin, params, waypoints, car, steps, opts, warm_opts, weights=None):
    """mpc_drive_twin with the arguments of mpc_drive_batch_host -> car, summary, hist [steps, 13, B], status, iters."""
    tx, ty = track_of(waypoints)
    car = _f(car).copy()
    B = car.shape[1]
    summary = np.full((NSUM, B), SENTINEL); hist = np.full((steps, REC, B), SENTINEL)
    status = np.full(B, ISENTINEL, dtype=np.int32); iters = np.full(B, ISENTINEL, dtype=np.int32)
    rc = twin.mpc_drive_twin(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(car), vp(tx), vp(ty), C.c_int(len(tx)), vp(_f(weights)),
                             C.byref(opts), C.byref(warm_opts), vp(summary), vp(hist), vp(status), vp(iters))
    assert rc == 0, rc
    return {"car": car, "summary": summary, "hist": hist, "status": status, "iters": iters}


def summary_from_hist(hist, n_track, cte_limit):
    """The summary rows recomputed from the records, in step order (a not-a-number never wins a maximum or the minimum)."""
    steps, _, B = hist.shape
    s = np.zeros((NSUM, B))
    s[4] = np.inf; s[6] = -1.0
    for t in range(steps):
        cte, epsi, speed = hist[t, REC_CTE], hist[t, REC_EPSI], hist[t, 3]
        ac, ae = np.abs(cte), np.abs(epsi)
        s[0] = np.where(ac > s[0], ac, s[0]); s[1] = s[1] + cte * cte; s[2] = np.where(ae > s[2], ae, s[2])
        s[3] = s[3] + speed; s[4] = np.where(speed < s[4], speed, s[4])
        if t > 0:
            d = (hist[t, REC_K] - hist[t - 1, REC_K]).astype(np.int64) % n_track
            s[5] += np.where(2 * d > n_track, d - n_track, d)
        s[6] = np.where((s[6] < 0) & (ac > cte_limit), float(t), s[6])
        s[7] += hist[t, REC_STATUS] != 0
    return s


def check_summary(res, n_track, cte_limit):
    """Rows 0, 2, 4, 5, 6, 7 equal; rows 1 and 3 -- running sums of `steps` terms -- within steps x 2 ulp of the sum."""
    hist, summary = res["hist"], res["summary"]
    ref = summary_from_hist(hist, n_track, cte_limit)
    for r in (0, 2, 4, 5, 6, 7):
        assert np.array_equal(summary[r], ref[r]), (r, summary[r], ref[r])
    for r in (1, 3):
        assert (np.abs(summary[r] - ref[r]) <= hist.shape[0] * 2 * np.spacing(np.abs(ref[r]))).all(), r
    assert np.array_equal(res["status"], hist[:, REC_STATUS].max(0).astype(np.int32))
    assert np.array_equal(res["iters"], hist[:, REC_ITERS].sum(0).astype(np.int32))


def oracle_check_steps(cfgname, over, params, waypoints, hist, extra, cars=None):
    """On every recorded step, the oracle's telemetry handler on the recorded car and window: the same status, the steer within
    TOL_STEER / max_steering and the throttle within 1e-5.  -> (max |d steer| [rad], max |d throttle|)."""
    steps, _, B = hist.shape
    cars = range(B) if cars is None else cars
    d_steer = d_thr = 0.0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in cars:
            cfg = O.load_config(cfgname, **over)          # run() mutates the yaw bounds of its Config, like the reference
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], extra)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            if st == 0:
                d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * params.max_steering)
                d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr
