"""Warm start on the run() path on the device (mpc_run_batch_device_warm / _host_warm, mpc_telemetry_batch_device_warm / _host_warm,
mpc_wire_telemetry_batch_host_warm, lib/mpc_replay --warm, MPC::run with setWarmStart): the warm wave kernel and the WARM build of
the lane kernel, the warm column read through mpc::WarmColumn, against the oracle's cold mpc_run on every step's own instance and
against the CPU build of the same functions (tests/host_twin, mpc_twin_run without a model array)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ
from run_warm_helpers import (build_drop_in_run_warm, closed_loop, load_run_warm_twin, oracle_runs, pick_window, plant, run_differences,
                              telemetry_pose, twin_closed_loop, twin_run)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return load_run_warm_twin()


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _device_loop(pkg, params, sc, waypoints, steps, dev, opts=None):
    """The handler loop through mpc_run_batch_device_warm, in place: one warm tensor and one status tensor for the whole loop (warm_in
    is warm_out, warm_status is status); step 1 has warm_in = NULL."""
    import torch
    B = sc["pose"].shape[1]
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        warm = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)

        def step(k, pose, px, py):
            r = mpc.run_torch(_t(pose, dev), _t(px, dev), _t(py, dev), warm=warm if k > 0 else None, warm_status=status if k > 0 else None,
                              warm_out=warm, status_out=status, warm_opts=opts)
            torch.cuda.synchronize()
            assert r["warm"] is warm and r["status"] is status
            return {k_: r[k_].cpu().numpy() for k_ in ("out8", "status", "iters")}
        return closed_loop(step, sc, waypoints, steps, params.max_steering)


def _check_loop(name, params, dev_rec, twin_rec, oracle, cars=None):
    """A device loop against the oracle's cold mpc_run on its own instances (the columns `cars`) and against the CPU build's loop."""
    ost, o8, oit = oracle
    sel = np.arange(dev_rec["status"].shape[1]) if cars is None else cars
    assert np.array_equal(dev_rec["status"][:, sel], ost), name                       # every status
    ok = ost == 0
    d = np.abs(dev_rec["out8"][:, :, sel] - o8)
    d_steer = (d[:, 4] * params.max_steering)[ok].max(); d_accel = d[:, 5][ok].max(); d_other = np.delete(d, (4, 5), axis=1).max(1)[ok].max()
    print("%s vs the oracle: max |d steer| %.3g rad, |d accel| %.3g, |d other| %.3g; iterations per warm solve %.2f (CPU build %.2f, oracle cold %.2f)" % (
        name, d_steer, d_accel, d_other, dev_rec["iters"][1:].mean(), twin_rec["iters"][1:].mean(), oit[1:].mean()))
    assert d_steer <= TOL_STEER and d_accel <= TOL_ACCEL and d_other <= TOL_TRAJ, name
    # the CPU build's loop: the same statuses on every solve, the same outputs within the tolerances (both loops are driven by their own
    # solver, and the device has its own sin / cos / division)
    assert np.array_equal(dev_rec["status"], twin_rec["status"]), name
    both = dev_rec["status"] == 0
    t = np.abs(dev_rec["out8"] - twin_rec["out8"])
    assert (t[:, 4] * params.max_steering)[both].max() <= TOL_STEER and t[:, 5][both].max() <= TOL_ACCEL and np.delete(t, (4, 5), axis=1).max(1)[both].max() <= TOL_TRAJ, name
    # warm solves take fewer iterations than the oracle's cold solves of the same instances
    assert dev_rec["iters"][1:][:, sel].sum() < oit[1:].sum(), name


def test_wave_path_closed_loop(pkg, twin, golden_dir, waypoints, torch_dev):
    cfgname, B, steps = "config-fast.json", 96, 8
    params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=122, filtered=True)
    dev = _device_loop(pkg, params, sc, waypoints, steps, torch_dev)
    tw = twin_closed_loop(twin, params, sc, waypoints, steps, pkg.warm_opts_default(), warm_start=True)
    _check_loop("wave, B = 96", params, dev, tw, oracle_runs(cfgname, {}, dev["pose"], dev["ptsx"], dev["ptsy"]))


def test_lane_warm_path_closed_loop(pkg, twin, golden_dir, waypoints, torch_dev):
    cfgname, B, steps = "config-fast.json", 2048, 3
    params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=122, filtered=True)
    dev = _device_loop(pkg, params, sc, waypoints, steps, torch_dev)
    tw = twin_closed_loop(twin, params, sc, waypoints, steps, pkg.warm_opts_default(), warm_start=True)
    cars = np.arange(0, B, 16)
    _check_loop("lane, B = 2048", params, dev, tw, oracle_runs(cfgname, {}, dev["pose"], dev["ptsx"], dev["ptsy"], cars), cars)


def test_long_horizon(pkg, twin, golden_dir, waypoints, torch_dev):
    cfgname, over, B, steps = "config-fast.json", dict(N=20, dt=0.05), 16, 4
    params = pkg.params_from_json(os.path.join(golden_dir, cfgname), f64_f32_start=0, **over)
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=122, filtered=True)
    dev = _device_loop(pkg, params, sc, waypoints, steps, torch_dev)
    tw = twin_closed_loop(twin, params, sc, waypoints, steps, pkg.warm_opts_default(), warm_start=True)
    _check_loop("N = 20", params, dev, tw, oracle_runs(cfgname, over, dev["pose"], dev["ptsx"], dev["ptsy"]))


def _ragged_calls(pkg, params, poses, windows, B, dev):
    """On a fresh handle, through the C ABI with ld = 16 and ld_warm = 24 > B: the cold run, the cold run through the warm entry point
    (warm_in = NULL) and a warm run of the next message in place.  Every output starts as a sentinel.  -> the arrays of the three calls."""
    import torch
    ld, ldw, F, I = 16, 24, -7777.25, -12345
    rows = pkg.warm_rows(params.N)

    def inp(a):
        a = np.asarray(a, dtype=np.float64)
        wide = np.zeros((a.shape[0], ld)); wide[:, :B] = a
        return _t(wide, dev)
    ff = lambda r, l=ld: torch.full((r, l), F, dtype=torch.float64, device=dev)
    ii = lambda: torch.full((ld,), I, dtype=torch.int32, device=dev)
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    got = []

    def fetch(**k):
        torch.cuda.synchronize()
        got.append({n: v.cpu().numpy().copy() for n, v in k.items()})
    p = lambda t: t.data_ptr()
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        pose, px, py = inp(poses[0]), inp(windows[0][0]), inp(windows[0][1])
        out8, traj, status, iters, pre = ff(8), ff(2 * params.N), ii(), ii(), ff(15)
        assert lib.mpc_run_batch_device(mpc._h, B, ld, 6, p(pose), p(px), p(py), p(out8), p(traj), p(status), p(iters), p(pre), stream) == 0, lib.mpc_last_error()
        fetch(out8=out8, traj=traj, status=status, iters=iters, pre=pre, ptsx=px)
        pose, px, py = inp(poses[0]), inp(windows[0][0]), inp(windows[0][1])
        out8, traj, status, iters, pre, warm = ff(8), ff(2 * params.N), ii(), ii(), ff(15), ff(rows, ldw)
        assert lib.mpc_run_batch_device_warm(mpc._h, B, ld, 6, p(pose), p(px), p(py), None, None, p(warm), ldw, None, p(out8), p(traj), p(status), p(iters),
                                             p(pre), stream) == 0, lib.mpc_last_error()
        fetch(out8=out8, traj=traj, status=status, iters=iters, pre=pre, ptsx=px, warm=warm)
        pose, px, py = inp(poses[1]), inp(windows[1][0]), inp(windows[1][1])
        out8, traj, iters, pre = ff(8), ff(2 * params.N), ii(), ff(15)
        assert lib.mpc_run_batch_device_warm(mpc._h, B, ld, 6, p(pose), p(px), p(py), p(warm), p(status), p(warm), ldw, None, p(out8), p(traj), p(status),
                                             p(iters), p(pre), stream) == 0, lib.mpc_last_error()
        fetch(out8=out8, traj=traj, status=status, iters=iters, pre=pre, ptsx=px, warm=warm)
    return got, F, I


@pytest.mark.parametrize("lpi", [16, 32, 64])
def test_ragged_batch_on_both_kernels(pkg, twin, golden_dir, waypoints, torch_dev, monkeypatch, lpi):
    """B = 7 with ld = 16 and ld_warm = 24 at 16, 32 and 64 lanes per instance: the warm wave kernel at every group size and the lane
    kernel's WARM build agree bitwise on the cold run, the cold run through the warm entry point and a warm run in place, and neither
    writes a column from B on."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    params.f64_f32_start = 0
    B = 7
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=122, filtered=True)
    w0 = pick_window(waypoints, sc["pose"][0], sc["pose"][1])
    first = twin_run(twin, params, sc["pose"], w0[0], w0[1], pkg.warm_opts_default())
    pose1 = plant(sc["pose"], first["out8"], params.max_steering)
    poses, windows = (sc["pose"], pose1), (w0, pick_window(waypoints, pose1[0], pose1[1]))
    monkeypatch.setenv("MPC_WAVE_LPI", str(lpi))
    res = {}
    for mode, limit in (("lane", "0"), ("wave", "1024")):
        monkeypatch.setenv("MPC_WAVE_MAX_BATCH", limit)       # (read when the handle is created)
        res[mode], F, I = _ragged_calls(pkg, params, poses, windows, B, torch_dev)
    names = ("cold", "cold through the warm entry point", "warm in place")
    for name, lane, wave in zip(names, res["lane"], res["wave"]):
        assert sorted(lane) == sorted(wave)
        for k in lane:
            for mode, a in (("lane", lane[k]), ("wave", wave[k])):
                if k != "ptsx":                               # (an input that is transformed in place: its padding is the caller's zeros)
                    assert (a[..., B:] == (I if a.dtype == np.int32 else F)).all(), (lpi, name, mode, k, "written beyond column B - 1")
            assert np.array_equal(lane[k][..., :B], wave[k][..., :B], equal_nan=True), (lpi, name, k)
        assert (lane["status"][:B] == 0).all(), (lpi, name)
    cold, viaw, warm = res["wave"]
    for k in ("out8", "traj", "status", "iters", "pre", "ptsx"):
        assert np.array_equal(cold[k], viaw[k], equal_nan=True), (lpi, k)
    assert warm["iters"][:B].sum() < cold["iters"][:B].sum()
    # ... and the warm run is the CPU build's warm run of the same message, from the same record
    tw = twin_run(twin, params, poses[1], windows[1][0], windows[1][1], pkg.warm_opts_default(), warm=first["warm"], warm_status=first["status"])
    assert np.array_equal(tw["status"], warm["status"][:B])
    d_steer, d_accel, d_other = run_differences(warm["out8"][:, :B], tw["out8"], params.max_steering)
    assert d_steer <= TOL_STEER and d_accel <= TOL_ACCEL and d_other <= TOL_TRAJ


@pytest.mark.parametrize("B", [96, 2048])
def test_cold_through_the_warm_entry_point_is_mpc_run_batch_device(pkg, golden_dir, waypoints, torch_dev, B):
    import torch
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=31)
    args = lambda: (_t(sc["pose"], torch_dev), _t(sc["ptsx"], torch_dev), _t(sc["ptsy"], torch_dev))
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        a = args(); cold = mpc.run_torch(*a, want_traj=True, want_pre=True)
        b = args(); w = mpc.run_torch(*b, want_traj=True, want_pre=True, want_warm=True)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        for k in ("out8", "status", "iters", "traj", "pre"):
            assert np.array_equal(cold[k].cpu().numpy(), w[k].cpu().numpy(), equal_nan=True), k
        ok = (w["status"] == 0).cpu().numpy()
        assert ok.mean() > 0.99 and np.isfinite(w["warm"].cpu().numpy()[:, ok]).all()
        # warm_status != SUCCESS and an all-NaN buffer: the cold run, bitwise
        for warm, ws in ((w["warm"], torch.full((B,), 2, dtype=torch.int32, device=torch_dev)), (torch.full_like(w["warm"], float("nan")), None)):
            c = args(); r = mpc.run_torch(*c, warm=warm, warm_status=ws)
            torch.cuda.synchronize()
            for k in ("out8", "status", "iters"):
                assert np.array_equal(cold[k].cpu().numpy(), r[k].cpu().numpy(), equal_nan=True), k


def test_telemetry_handler_warm(pkg, twin, golden_dir, waypoints, torch_dev):
    """mpc_telemetry_batch_device_warm over four messages per car, in place, every reply against the oracle's telemetry_handler on the
    same message; the host and the wire form give the device form's numbers."""
    import torch
    cfgname, B, steps = "config-fast.json", 64, 4
    params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=122, latency_s=0.0)
    lib = pkg.library()
    tel = np.stack([sc["pose"][0], sc["pose"][1], sc["pose"][2], np.minimum(sc["pose"][3], 0.8 * params.max_speed) * 3600.0 / 1609.34, -sc["pose"][4],
                    np.zeros(B)])
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        warm = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=torch_dev)
        status = torch.empty((B,), dtype=torch.int32, device=torch_dev)
        hwarm, hstatus = None, None
        for k in range(steps):
            px, py = pick_window(waypoints, tel[0], tel[1])
            # the host form first, from the host copy of the same record (separate buffers)
            hcmd = np.zeros((2, B)); hst = np.zeros(B, dtype=np.int32); hw = np.zeros((mpc.warm_rows(), B))
            v = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
            telc = np.ascontiguousarray(tel)
            assert lib.mpc_telemetry_batch_host_warm(mpc._h, B, B, 6, v(telc), 0.0, v(px), v(py), v(hwarm), v(hstatus), v(hw), B, None, v(hcmd), v(hst)) == 0, lib.mpc_last_error()
            r = mpc.telemetry_torch(_t(tel, torch_dev), _t(px, torch_dev), _t(py, torch_dev), want_out8=True, warm=warm if k > 0 else None,
                                    warm_status=status if k > 0 else None, warm_out=warm, status_out=status)
            torch.cuda.synchronize()
            cmd, st, out8 = r["cmd"].cpu().numpy(), r["status"].cpu().numpy(), r["out8"].cpu().numpy()
            assert np.array_equal(hcmd, cmd) and np.array_equal(hst, st) and np.array_equal(hw, warm.cpu().numpy(), equal_nan=True)
            hwarm, hstatus = hw, hst
            for i in range(B):
                cfg = O.load_config(cfgname)
                ost, ref_steer, ref_thr, o8 = O.telemetry_handler(cfg, list(tel[:, i]), list(px[:, i]), list(py[:, i]), 0.0)
                assert ost == st[i], (k, i)
                if ost == 0:
                    assert abs(cmd[0, i] - ref_steer) * params.max_steering <= TOL_STEER and abs(cmd[1, i] - ref_thr) <= 1e-5, (k, i)
                    d = np.abs(out8[:, i] - o8)
                    assert d[4] * params.max_steering <= TOL_STEER and d[5] <= TOL_ACCEL and np.delete(d, (4, 5)).max() <= TOL_TRAJ, (k, i)
            # the next message: the car at the step-1 state of the compensated pose, the reply as the previous throttle
            pose = plant(telemetry_pose(params, tel), out8, params.max_steering)
            tel = np.stack([pose[0], pose[1], pose[2], pose[3] * 3600.0 / 1609.34, cmd[0] * params.max_steering, cmd[1]])
        # (iterations of the telemetry entry point are not returned: one more warm message through run_torch's twin, from the final record)
        px, py = pick_window(waypoints, tel[0], tel[1])
        last_cold = twin_run(twin, params, tel, px, py, pkg.warm_opts_default(), tel=True)
        last_warm = twin_run(twin, params, tel, px, py, pkg.warm_opts_default(), tel=True, warm=warm.cpu().numpy(), warm_status=status.cpu().numpy())
        print("telemetry, message 5 from the device's record (CPU build): iterations cold %d, warm %d" % (last_cold["iters"].sum(), last_warm["iters"].sum()))
        assert last_warm["iters"].sum() < last_cold["iters"].sum()
        # the wire form: the same message as parsed frames
        W = (pkg.MpcWireTelemetry * B)()
        for i in range(B):
            W[i].x, W[i].y, W[i].psi, W[i].speed, W[i].steering_angle, W[i].throttle, W[i].npts = tel[0, i], tel[1, i], tel[2, i], tel[3, i], tel[4, i], 0.0, 6
            for q in range(6):
                W[i].ptsx[q] = px[q, i]; W[i].ptsy[q] = py[q, i]
        prev = np.ascontiguousarray(tel[5])
        wcmd = np.zeros((2, B)); wst = np.zeros(B, dtype=np.int32); ww = hwarm.copy(); wws = hstatus.copy()
        assert lib.mpc_wire_telemetry_batch_host_warm(mpc._h, B, W, v(prev), 0.0, v(ww), v(wws), v(ww), B, None, v(wcmd), v(wst)) == 0, lib.mpc_last_error()
        hcmd = np.zeros((2, B)); hst = np.zeros(B, dtype=np.int32); hw = np.zeros_like(hwarm)
        telc = np.ascontiguousarray(tel)
        assert lib.mpc_telemetry_batch_host_warm(mpc._h, B, B, 6, v(telc), 0.0, v(px), v(py), v(hwarm), v(hstatus), v(hw), B, None, v(hcmd), v(hst)) == 0
        assert np.array_equal(wcmd, hcmd) and np.array_equal(wst, hst) and np.array_equal(ww, hw, equal_nan=True)
        assert np.array_equal(hst, last_warm["status"])


@pytest.mark.parametrize("B", [1, 300])
def test_host_entry_point(pkg, twin, golden_dir, waypoints, torch_dev, B):
    """mpc_run_batch_host_warm over three messages: the oracle on a sample, the CPU build's statuses on all."""
    cfgname, steps = "config-fast.json", 3
    params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=122, filtered=True)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        mem = {"warm": None, "status": None}

        def step(k, pose, px, py):
            r = mpc.run_numpy(pose, px, py, warm=mem["warm"], warm_status=mem["status"], want_warm=True)
            mem["warm"], mem["status"] = r["warm"], r["status"]
            return r
        dev = closed_loop(step, sc, waypoints, steps, params.max_steering)
        cold = mpc.run_numpy(dev["pose"][0], dev["ptsx"][0], dev["ptsy"][0])
        assert np.array_equal(cold["out8"], dev["out8"][0]) and np.array_equal(cold["iters"], dev["iters"][0])        # warm_in = NULL: the cold entry point
    tw = twin_closed_loop(twin, params, sc, waypoints, steps, pkg.warm_opts_default(), warm_start=True)
    cars = np.arange(0, B, 10)
    _check_loop("host, B = %d" % B, params, dev, tw, oracle_runs(cfgname, {}, dev["pose"], dev["ptsx"], dev["ptsy"], cars), cars)


def test_refusals(pkg, golden_dir, waypoints, torch_dev):
    import torch
    lib = pkg.library()
    B = 32

    def calls(params):
        sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=5)
        rows = pkg.warm_rows(params.N)
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            pose, px, py = _t(sc["pose"], torch_dev), _t(sc["ptsx"], torch_dev), _t(sc["ptsy"], torch_dev)
            px2, py2 = _t(sc["ptsx"], torch_dev), _t(sc["ptsy"], torch_dev)       # (the waypoints are transformed in place)
            w = torch.zeros((rows, B), dtype=torch.float64, device=torch_dev); st = torch.zeros(B, dtype=torch.int32, device=torch_dev)
            o8 = torch.zeros((8, B), dtype=torch.float64, device=torch_dev); cmd = torch.zeros((2, B), dtype=torch.float64, device=torch_dev)
            p = lambda t: t.data_ptr()
            rc = [lib.mpc_run_batch_device_warm(mpc._h, B, B, 6, p(pose), p(px), p(py), None, None, p(w), B, None, p(o8), None, p(st), None, None, None)]
            msg = lib.mpc_last_error()
            rc.append(lib.mpc_telemetry_batch_device_warm(mpc._h, B, B, 6, p(pose), 0.0, p(px2), p(py2), None, None, p(w), B, None, p(cmd), None, p(st), None))
            h = lambda a: C.c_void_p(a.ctypes.data)
            hp, hx, hy = (np.ascontiguousarray(sc[k]) for k in ("pose", "ptsx", "ptsy"))
            hw = np.zeros((rows, B)); ho = np.zeros((8, B)); hc = np.zeros((2, B)); hs = np.zeros(B, dtype=np.int32)
            rc.append(lib.mpc_run_batch_host_warm(mpc._h, B, B, 6, h(hp), h(hx), h(hy), None, None, h(hw), B, None, h(ho), None, h(hs), None, None))
            rc.append(lib.mpc_telemetry_batch_host_warm(mpc._h, B, B, 6, h(hp), 0.0, h(hx), h(hy), None, None, h(hw), B, None, h(hc), h(hs)))
            rc.append(lib.mpc_run_batch_device_warm(mpc._h, B, B, 6, p(pose), p(px2), p(py2), None, None, p(w), B - 1, None, p(o8), None, p(st), None, None, None))
            torch.cuda.synchronize()
        return rc, msg
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    rc, _ = calls(params)
    assert rc == [0, 0, 0, 0, -1]
    q = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), N=15, dt=0.05)      # f64_f32_start on at N >= 15: two launches
    rc, msg = calls(q)
    assert rc[:4] == [-4] * 4 and b"f64_f32_start" in msg
    q = params.copy(); q.max_soc = 4
    rc, msg = calls(q)
    assert rc[:4] == [-4] * 4 and b"max_soc" in msg


def test_drop_in_run_warm_start(pkg, golden_dir, tmp_path):
    exe = build_drop_in_run_warm(pkg, str(tmp_path))
    r = subprocess.run([exe, os.path.join(golden_dir, "config-stable.json"), "10"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    params = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"))
    rows = {"cold": [], "warm": []}; total = {}
    for l in r.stdout.strip().splitlines():
        p = l.split()
        if p[1] == "total":
            total[p[0]] = int(p[2])
        else:
            rows[p[0]].append([float(x) for x in p[2:]])
    cold, warm = np.array(rows["cold"]), np.array(rows["warm"])
    assert cold.shape == warm.shape == (10, 9)
    print("MPC::run() x 10: iterations cold %d, warm %d" % (total["cold"], total["warm"]))
    d = np.abs(warm[:, 1:] - cold[:, 1:])
    assert d[:, 4].max() * params.max_steering <= TOL_STEER and d[:, 5].max() <= TOL_ACCEL and np.delete(d, (4, 5), axis=1).max() <= TOL_TRAJ
    assert warm[0, 0] == cold[0, 0] and total["warm"] < total["cold"]


def test_replay_tool_warm(pkg, golden_dir, waypoints):
    """lib/mpc_replay --warm on the frames of tests/test_wire.py's replay: the replies of the run without the flag, within that test's
    tolerances; without the flag nothing changed (that test compares those replies with the oracle)."""
    from test_wire import _frames_for
    cfgname = "config-fast.json"
    params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
    B = 48
    f1, _, _ = _frames_for(pkg, params, waypoints, B, 71)
    f2, rows2, tel2 = _frames_for(pkg, params, waypoints, B, 72)
    text = "\n".join(f1 + ['42["telemetry",null]'] * B + f2 + f2) + "\n"
    exe = os.path.join(os.path.dirname(pkg.library_path()), "mpc_replay")
    outs = []
    for flags in ([], ["--warm"]):
        p = subprocess.run([exe, os.path.join(golden_dir, cfgname), "--cars", str(B)] + flags, input=text, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        outs.append(p.stdout.splitlines())
    plain, warm = outs
    assert len(plain) == len(warm) == 4 * B and plain[:B] == warm[:B] and warm[B:2 * B] == ['42["manual",{}]'] * B      # a car's first message is cold
    compared = 0
    for n, (a, b) in enumerate(zip(plain[2 * B:], warm[2 * B:])):
        da, db = json.loads(a[2:])[1], json.loads(b[2:])[1]
        # as in that test: a message the oracle's handler does not solve carries no tolerance (a warm attempt may solve it)
        i = n % B
        prev = json.loads(plain[n + B][2:])[1]["throttle"] if n >= B else 0.0
        st = O.telemetry_handler(O.load_config(cfgname), [rows2[0, i], rows2[1, i], rows2[2, i], rows2[3, i], rows2[4, i], prev], list(tel2["ptsx"][:, i]),
                                 list(tel2["ptsy"][:, i]), 0.0)[0]
        if st != 0:
            continue
        compared += 1
        assert abs(da["steering_angle"] - db["steering_angle"]) * params.max_steering < 5 * TOL_STEER and abs(da["throttle"] - db["throttle"]) < 1e-5
    assert compared > 1.8 * B
