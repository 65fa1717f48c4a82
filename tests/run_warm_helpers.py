"""Helpers of the run()-path warm-start tests (test infrastructure): the TEST-ONLY CPU build (mpc_twin_run and mpc_twin_solve of tests/host_twin), the closed
loop of a telemetry handler (window rule, ideal plant) that both test files and the tools drive, and the oracle's cold mpc_run on
every step's instance -- the comparison is solve by solve, so loop amplification and window flips cannot enter."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
from helpers import ROOT, load_twin, vp

NPTS = 6
load_run_warm_twin = load_twin


def pick_window(wp, x, y, npts=NPTS):
    """Six waypoints per car, starting at the waypoint just behind it: j = the waypoint nearest to the car, k = j if
    (p - wp[j]) . (wp[j+1] - wp[j]) > 0 else j - 1; the window is wp[k .. k+5] cyclically.  -> ptsx, ptsy [npts, B]."""
    wp = np.asarray(wp, dtype=np.float64)
    n = len(wp)
    p = np.stack([x, y], axis=1)
    j = np.argmin(((p[:, None, :] - wp[None, :, :]) ** 2).sum(2), axis=1)
    ahead = ((p - wp[j]) * (wp[(j + 1) % n] - wp[j])).sum(1) > 0
    k = np.where(ahead, j, j - 1)
    idx = (k[None, :] + np.arange(npts)[:, None]) % n
    return np.ascontiguousarray(wp[idx, 0]), np.ascontiguousarray(wp[idx, 1])


def plant(pose, out8, max_steering):
    """The ideal plant: the car moves to the solution's step-1 state, out8 = (x1, y1, psi1, v1, steer, accel, ...) in the vehicle
    frame.  -> the next pose [6, B]."""
    x, y, psi = pose[0], pose[1], pose[2]
    c, s = np.cos(psi), np.sin(psi)
    return np.stack([x + out8[0] * c - out8[1] * s, y + out8[0] * s + out8[1] * c, psi + out8[2], out8[3], out8[4] * max_steering, out8[5]])


def twin_run(twin, params, pose, ptsx, ptsy, opts, warm=None, warm_status=None, tel=False, extra=0.0):
    """mpc_twin_run without per-instance model values, with the arguments of mpc_run_batch_host_warm (tel: of mpc_telemetry_batch_host_warm, `pose` = the
    telemetry rows) -> out8, cmd, status, iters, pre, warm."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    pose, px, py = f(pose), f(ptsx).copy(), f(ptsy).copy()          # (the waypoints are transformed in place: the caller keeps its own)
    B, npts = pose.shape[1], px.shape[0]
    rows = (params.N - 1) * 22
    out8 = np.zeros((8, B)); cmd = np.zeros((2, B)); pre = np.zeros((15, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    wout = np.zeros((rows, B))
    if warm is not None:
        warm = f(warm)
        assert warm.shape == (rows, B)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_twin_run(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(npts), vp(pose), C.c_int(1 if tel else 0), C.c_double(extra),
                           vp(px), vp(py), None, vp(warm), vp(warm_status), vp(wout), C.c_int64(B), C.byref(opts), vp(out8), vp(cmd), vp(status),
                           vp(iters), vp(pre))
    assert rc == 0
    return {"out8": out8, "cmd": cmd, "status": status, "iters": iters, "pre": pre, "warm": wout}


def twin_solve_box(twin, params, batch, opts, psi_box, warm=None, warm_status=None):
    """The solve inside run() on its own (the psi box posed by the caller): psi_box = True reads the warm buffer the way the run()
    path does, False the way mpc_solve_batch_host_warm does."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh = f(batch["state"]), f(batch["coeffs"]), f(batch["yaw_lo"]), f(batch["yaw_hi"])
    B = st.shape[1]
    rows = (params.N - 1) * 22
    out = np.zeros((9, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32); wout = np.zeros((rows, B))
    if warm is not None:
        warm = f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_twin_solve(C.byref(params), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), None, None, vp(warm), vp(warm_status),
                             vp(wout), C.c_int64(B), C.byref(opts), C.c_int(1 if psi_box else 0), vp(out), None, vp(status), vp(iters))
    assert rc == 0
    return {"out": out, "status": status, "iters": iters, "warm": wout}


def closed_loop(step, sc, waypoints, steps, max_steering, between=None):
    """The handler loop for the cars of `sc` (a lake_track_batch): every step picks the window, calls step(k, pose, ptsx, ptsy)
    -> dict with out8 [8, B], status, iters (numpy), and moves the cars with the ideal plant.  `between(k)`: called after the plant
    (the tools re-frame the warm buffer there).  -> the record of every solve: pose [steps, 6, B], ptsx / ptsy [steps, 6, B], out8
    [steps, 8, B], status and iters [steps, B]."""
    pose = np.array(sc["pose"], dtype=np.float64, copy=True)
    B = pose.shape[1]
    rec = {"pose": np.zeros((steps, 6, B)), "ptsx": np.zeros((steps, NPTS, B)), "ptsy": np.zeros((steps, NPTS, B)), "out8": np.zeros((steps, 8, B)),
           "status": np.zeros((steps, B), dtype=np.int32), "iters": np.zeros((steps, B), dtype=np.int32)}
    for k in range(steps):
        px, py = pick_window(waypoints, pose[0], pose[1])
        r = step(k, pose, px, py)
        rec["pose"][k] = pose; rec["ptsx"][k] = px; rec["ptsy"][k] = py
        rec["out8"][k] = r["out8"]; rec["status"][k] = r["status"]; rec["iters"][k] = r["iters"]
        pose = plant(pose, r["out8"], max_steering)
        if between is not None:
            between(k)
    return rec


def twin_closed_loop(twin, params, sc, waypoints, steps, opts, warm_start):
    """closed_loop driven by the CPU build: step 1 cold, the others warm-started from the step before (or cold too)."""
    mem = {"warm": None, "status": None}

    def step(k, pose, px, py):
        r = twin_run(twin, params, pose, px, py, opts, warm=mem["warm"] if warm_start else None, warm_status=mem["status"] if warm_start else None)
        mem["warm"], mem["status"] = r["warm"], r["status"]
        return r
    return closed_loop(step, sc, waypoints, steps, params.max_steering)


def oracle_runs(cfgname, over, pose, ptsx, ptsy, cars=None):
    """The oracle's cold mpc_run on recorded instances: pose [steps, 6, B], ptsx / ptsy [steps, npts, B] (cars: the columns to solve,
    default all) -> status [steps, n], out8 [steps, 8, n], iterations [steps, n]."""
    steps, _, B = pose.shape
    cars = np.arange(B) if cars is None else np.asarray(cars)
    status = np.zeros((steps, len(cars)), dtype=np.int32); out8 = np.zeros((steps, 8, len(cars))); iters = np.zeros((steps, len(cars)), dtype=np.int32)
    for k in range(steps):
        for n, i in enumerate(cars):
            cfg = O.load_config(cfgname, **over)          # run() mutates the yaw bounds of its Config, like the reference
            st, o8, _, _, _, info = O.mpc_run(cfg, pose[k, :, i], ptsx[k, :, i], ptsy[k, :, i])
            status[k, n] = st; out8[k, :, n] = o8; iters[k, n] = info.iterations
    return status, out8, iters


def run_differences(out8, ref8, max_steering):
    """max |d steer| [rad], |d accel|, |d of the other six rows| between two out8 arrays [..., 8, n]."""
    d = np.abs(np.asarray(out8) - np.asarray(ref8))
    other = np.delete(d, (4, 5), axis=-2)
    return float(d[..., 4, :].max() * max_steering), float(d[..., 5, :].max()), float(other.max())


def build_drop_in_run_warm(pkg, out_dir=None):
    """Compile tests/cpp/drop_in_run_warm_test.cpp against include/mpc_drop_in.hpp and the product library -> path of the binary."""
    import tempfile
    pkg.library()
    out = os.path.join(out_dir or tempfile.mkdtemp(prefix="dropin_run_warm"), "drop_in_run_warm_test")
    libdir = os.path.dirname(pkg.library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "drop_in_run_warm_test.cpp"), "-L", libdir, "-lmpc_amd", "-Wl,-rpath," + libdir])
    return out


def telemetry_pose(params, tel, extra=0.0):
    """The pose the handler hands to run() for telemetry rows [6, B] (mpc_main.cpp:126-159: units, sign, latency compensation), in
    numpy: only to move the cars of a telemetry loop on; the comparison never uses it."""
    x, y, psi, mph, sa, thr = [np.asarray(t, dtype=np.float64) for t in tel]
    psi = (psi + np.pi) % (2 * np.pi) - np.pi
    v = mph * 1609.34 / 3600.0
    steer, acc = -sa, (thr - v / 50.0) * 6.0
    if params.latency_ms != 0:
        dtm = params.lookahead + extra
        dist = v * dtm
        return np.stack([x + dist * np.cos(psi), y + dist * np.sin(psi), psi + steer * dist / params.Lf, v + acc * dtm, steer, acc])
    return np.stack([x, y, psi, v, steer, acc])
