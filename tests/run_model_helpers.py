"""Helpers of the tests of run() and the telemetry handler with per-instance model values (test infrastructure): the TEST-ONLY CPU
build (mpc_twin_run of tests/host_twin), the stated population -- 48 lake-track cars, each with a column of its own --, and the oracle's mpc_run /
telemetry_handler with a per-car OrcConfig: the yardstick of these tests."""
import ctypes as C

import numpy as np

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, load_twin, vp
from model_helpers import MODEL_FIELDS, draw_rows

NPTS = 6
FLEET_B = 48
TOL_THROTTLE = 1e-5          # the throttle tolerance of the telemetry tests (tests/test_run_warm_gpu.py, tests/test_wire.py)
EXTRA_LATENCY = 0.02
INFEASIBLE = 3               # MPC_STATUS_INFEASIBLE


load_run_model_twin = load_twin


def fleet(pkg, params, waypoints, B=FLEET_B):
    """The stated population: lake_track_batch(48, seed 77) with the columns draw_rows(48, seed 9) -> pose [6, B], ptsx / ptsy
    [6, B], model [6, B] and the telemetry rows of the same cars (x, y, psi of the pose; v in mph; the steering sign flipped;
    previous throttle 0.3)."""
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=77)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    pose, px, py = f(sc["pose"]), f(sc["ptsx"]), f(sc["ptsy"])
    assert px.shape[0] == NPTS
    tel = f(np.stack([pose[0], pose[1], pose[2], pose[3] * 3600.0 / 1609.34, -pose[4], np.full(B, 0.3)]))
    return {"pose": pose, "ptsx": px, "ptsy": py, "tel": tel, "model": draw_rows(params, B, seed=9)}


def uniform_model(params, B):
    """every column the handle's own values"""
    return np.ascontiguousarray(np.repeat(np.array([[getattr(params, k)] for k in MODEL_FIELDS], dtype=np.float64), B, axis=1))


def twin_run_model(twin, params, pose, ptsx, ptsy, model, opts, warm=None, warm_status=None, tel=False, extra=0.0):
    """mpc_twin_run with the arguments of mpc_run_batch_host_warm_model (tel: of mpc_telemetry_batch_host_warm_model, `pose` =
    the telemetry rows) -> out8, cmd, status, iters, pre, warm and the vehicle-frame waypoints."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    pose, px, py, md = f(pose), f(ptsx).copy(), f(ptsy).copy(), f(model)
    B, npts = pose.shape[1], px.shape[0]
    assert md.shape == (6, B)
    rows = (params.N - 1) * 22
    out8 = np.zeros((8, B)); cmd = np.zeros((2, B)); pre = np.zeros((15, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    wout = np.zeros((rows, B))
    if warm is not None:
        warm = f(warm)
        assert warm.shape == (rows, B)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_twin_run(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(npts), vp(pose), C.c_int(1 if tel else 0), C.c_double(extra),
                           vp(px), vp(py), vp(md), vp(warm), vp(warm_status), vp(wout), C.c_int64(B), C.byref(opts), vp(out8), vp(cmd),
                           vp(status), vp(iters), vp(pre))
    assert rc == 0
    return {"out8": out8, "cmd": cmd, "status": status, "iters": iters, "pre": pre, "warm": wout, "ptsx": px, "ptsy": py}


def car_config(cfgname, model, i, **over):
    """the oracle's Config of car i: the handle's file with the six values of its column"""
    over = dict(over)
    over.update({name: float(model[q, i]) for q, name in enumerate(MODEL_FIELDS)})
    return O.load_config(cfgname, **over)


def oracle_fleet(cfgname, pose, ptsx, ptsy, model, tel=False, extra=0.0, cars=None):
    """The oracle on every car (or the columns `cars`) with its own OrcConfig: mpc_run on the poses, or telemetry_handler on the
    telemetry rows -> status, out8 [8, n], cmd [2, n] (telemetry), iters, and what run() derived before the solve: target speed, psi
    box, max_yaw_change (rows 14, 11, 12, 13 of `pre`) and the vehicle-frame waypoints."""
    B = pose.shape[1]
    cars = np.arange(B) if cars is None else np.asarray(cars)
    n = len(cars)
    res = {"status": np.zeros(n, dtype=np.int32), "out8": np.zeros((8, n)), "cmd": np.zeros((2, n)), "iters": np.zeros(n, dtype=np.int32),
           "pre": np.full((15, n), np.nan), "ptsx": np.zeros((ptsx.shape[0], n)), "ptsy": np.zeros((ptsx.shape[0], n))}
    for j, i in enumerate(cars):
        cfg = car_config(cfgname, model, i)              # (a fresh one per call: run() mutates the yaw bounds of its Config)
        if tel:
            st, steer, thr, o8 = O.telemetry_handler(cfg, list(pose[:, i]), list(ptsx[:, i]), list(ptsy[:, i]), extra)
            res["cmd"][:, j] = (steer, thr)
        else:
            st, o8, _, _, pre, info = O.mpc_run(cfg, pose[:, i], ptsx[:, i], ptsy[:, i])
            res["iters"][j] = info.iterations
            res["pre"][:6, j] = list(pre.state); res["pre"][6:11, j] = list(pre.coef)[:5]
            res["pre"][11, j] = pre.yaw_low; res["pre"][12, j] = pre.yaw_high; res["pre"][13, j] = pre.max_yaw_change; res["pre"][14, j] = pre.target_speed
            _, vx, vy = O.run_pre(car_config(cfgname, model, i), pose[:, i], ptsx[:, i], ptsy[:, i])
            res["ptsx"][:, j] = vx; res["ptsy"][:, j] = vy
        res["status"][j] = st; res["out8"][:, j] = o8
    return res


def assert_fleet_matches_oracle(got, ref, model, tel=False, cars=None, what="", min_converged=40):
    """The condition of every oracle comparison: the oracle's status on every car; every car it converges on within TOL_STEER on steer
    x the car's own max_steering, TOL_ACCEL, TOL_TRAJ on the other rows of out8 and -- telemetry -- the throttle tolerance; none left
    out; at least `min_converged` converge."""
    n = ref["status"].shape[0]
    cars = np.arange(n) if cars is None else np.asarray(cars)
    gs = np.asarray(got["status"])[cars]
    assert np.array_equal(gs, ref["status"]), (what, "status differs at", cars[gs != ref["status"]].tolist(), gs[gs != ref["status"]].tolist())
    ok = ref["status"] == 0
    assert ok.sum() >= min_converged, (what, int(ok.sum()))
    ms = np.asarray(model)[2, cars]
    line = "%s vs the oracle: %d of %d converged" % (what, int(ok.sum()), n)
    if got.get("out8") is not None:
        d = np.abs(np.asarray(got["out8"])[:, cars] - ref["out8"])
        d_steer = (d[4] * ms)[ok].max(); d_accel = d[5][ok].max(); d_other = np.delete(d, (4, 5), axis=0)[:, ok].max()
        line += ", max |d steer| %.3g rad, |d accel| %.3g, |d other| %.3g" % (d_steer, d_accel, d_other)
    if tel:
        c = np.abs(np.asarray(got["cmd"])[:, cars] - ref["cmd"])
        c_steer = (c[0] * ms)[ok].max(); c_thr = c[1][ok].max()
        line += ", reply: |d steer| %.3g rad, |d throttle| %.3g" % (c_steer, c_thr)
    print(line)
    if got.get("out8") is not None:
        assert d_steer <= TOL_STEER and d_accel <= TOL_ACCEL and d_other <= TOL_TRAJ, (what, d_steer, d_accel, d_other)
        assert np.isfinite(np.asarray(got["out8"])[:, cars]).all(), what
    if tel:
        assert c_steer <= TOL_STEER and c_thr <= TOL_THROTTLE, (what, c_steer, c_thr)
        assert np.isfinite(np.asarray(got["cmd"])[:, cars]).all(), what


def assert_pre_matches_oracle(got, ref, what=""):
    """`pre` and the vehicle-frame waypoints against what the oracle's run() derived with the car's own Config: the state, the fit,
    the psi box, max_yaw_change and the target speed -- the rows the car's own max_speed decides are 14 (and nothing else: the box
    comes from the fit)."""
    d = np.abs(got["pre"] - ref["pre"])
    print("%s pre vs the oracle: max |d| state %.3g, coeffs %.3g, box %.3g, target speed %.3g" % (what, d[:6].max(), d[6:11].max(), d[11:14].max(), d[14].max()))
    assert d[:6].max() <= 1e-9 and d[6:11].max() <= 1e-9 and d[11:14].max() <= 1e-9 and d[14].max() <= 1e-9, what
    assert np.abs(got["ptsx"] - ref["ptsx"]).max() <= 1e-9 and np.abs(got["ptsy"] - ref["ptsy"]).max() <= 1e-9, what
