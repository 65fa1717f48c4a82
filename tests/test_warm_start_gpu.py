"""Warm start on the device (mpc_solve_batch_device_warm / _host_warm / mpc_rollout_batch_device_warm, MPC::setWarmStart): the WARM
build of the lane kernel and the warm wave kernel against the CPU build of the same Solver functions (tests/host_twin, mpc_twin_solve), the cold
entry points and the oracle's cold closed loops."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, closed_loop_report
from warm_helpers import build_drop_in_warm, load_warm_twin, twin_closed_loop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def warm_twin():
    return load_warm_twin()


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items() if v is not None}


def test_cold_through_the_warm_entry_point_is_the_cold_solve(pkg, golden_dir, waypoints, torch_dev):
    """warm_in = NULL on 8192 instances (the lane kernel's WARM build): bitwise mpc_solve_batch_device."""
    import torch
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    assert params.tail_cut == 0
    B = 8192
    b = pkg.scenarios.lake_track_batch(B, params, waypoints)
    ins = [_t(b[k], torch_dev) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")]
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        cold = mpc.solve_torch(*ins, want_traj=True)
        torch.cuda.synchronize()
        cold = _np(cold)
        w = mpc.solve_torch(*ins, want_traj=True, want_warm=True)
        torch.cuda.synchronize()
        w = _np(w)
    assert (cold["status"] == 0).mean() > 0.99
    for k in ("status", "iters", "out", "traj"):
        assert np.array_equal(cold[k], w[k], equal_nan=True), k
    assert w["warm"].shape == (pkg.warm_rows(params.N), B) and np.isfinite(w["warm"][:, cold["status"] == 0]).all()
    # the iterate that came out is the point that was reported: record 0 holds the step-1 state and the first controls
    ok = cold["status"] == 0
    # (out is projected into the caller's bounds, the iterate lies within the relaxed ones: 1e-8 relative)
    assert np.abs(w["warm"][:6][:, ok] - cold["out"][:6][:, ok]).max() <= 1e-6 and np.abs(w["warm"][6:8][:, ok] - cold["out"][6:8][:, ok]).max() <= 1e-6


def _device_loop(pkg, params, sc, idx, steps, dev, inplace=True):
    """The closed loop of tests/test_warm_start.py on the device for the cars idx (tiled): step 1 cold, then warm, in place."""
    import torch
    B = len(idx)
    state = _t(sc["state"][:, idx], dev)
    coeffs, ylo, yhi = _t(sc["coeffs"][:, idx], dev), _t(sc["yaw_lo"][idx], dev), _t(sc["yaw_hi"][idx], dev)
    hist = np.zeros((steps, 9, B)); sst = np.zeros((steps, B), dtype=np.int32); sit = np.zeros((steps, B), dtype=np.int32)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        outputs = mpc.alloc_outputs(B, dev)
        warm = None
        for k in range(steps):
            r = mpc.solve_torch(state, coeffs, ylo, yhi, outputs=outputs, warm=warm, warm_status=outputs["status"] if warm is not None else None,
                                want_warm=True)
            torch.cuda.synchronize()
            hist[k] = r["out"].cpu().numpy(); sst[k] = r["status"].cpu().numpy(); sit[k] = r["iters"].cpu().numpy()
            state = r["out"][:6].clone().contiguous()
            warm = r["warm"]                       # (the same tensor every step: warm_in is warm_out, warm_status is status)
    return hist, sst, sit


def test_closed_loops_warm_on_both_kernels(pkg, warm_twin, golden_dir, waypoints, torch_dev):
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    cars, steps = 96, 25
    sc = pkg.scenarios.lake_track_batch(cars, params, waypoints, seed=122)
    opts = pkg.warm_opts_default()
    th, tst, tit = twin_closed_loop(warm_twin, params, sc, steps, opts, warm_start=True)
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    _, oh, ost = O.rollout_chunk_full(("config-fast.json", {}, c(sc["state"]), c(sc["coeffs"]), c(sc["yaw_lo"]), c(sc["yaw_hi"]), steps))
    res = {}
    for name, idx in (("lane", np.arange(4096) % cars), ("wave96", np.arange(cars)), ("wave1", np.array([5]))):
        hist, sst, sit = _device_loop(pkg, params, sc, idx, steps, torch_dev)
        res[name] = (hist, sst, sit)
        assert np.array_equal(sst, tst[:, idx]), name                           # every solve: the CPU build's status
        cl = closed_loop_report(hist, sst, oh[:, :, idx], ost[:, idx])
        print(name, "max |d steer| %.3g |d accel| %.3g |d state| %.3g, iterations per warm solve %.2f (CPU build %.2f)" % (
            cl["d_steer_rad"][3], cl["d_accel"][3], cl["d_state"][3], sit[1:].mean(), tit[1:][:, idx].mean()))
        assert cl["status_differs"] == 0 and cl["cars_on_another_local_minimum"] == 0, (name, cl)
        assert cl["d_steer_rad"][3] <= TOL_STEER and cl["d_accel"][3] <= TOL_ACCEL and cl["d_state"][3] <= TOL_TRAJ, (name, cl)
    # lane kernel and wave kernel: bitwise, as tests/test_gpu_parity.py asks of them for cold solves
    lane, w96, w1 = res["lane"], res["wave96"], res["wave1"]
    for q, what in enumerate(("out", "status", "iters")):
        assert np.array_equal(lane[q][..., :cars], w96[q], equal_nan=True), what
        assert np.array_equal(lane[q][..., cars:2 * cars], w96[q], equal_nan=True), what      # the tiled copies too
        assert np.array_equal(w96[q][..., 5:6], w1[q], equal_nan=True), what


def test_warm_rollout_entry_point(pkg, golden_dir, waypoints, torch_dev):
    import torch
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    cfg = O.load_config("config-fast.json")
    B, steps = 1024, 6
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=61)
    args = lambda: (_t(sc["state"], torch_dev), _t(sc["coeffs"], torch_dev), _t(sc["yaw_lo"], torch_dev), _t(sc["yaw_hi"], torch_dev))
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        cold = mpc.rollout_torch(*args(), steps=steps)
        torch.cuda.synchronize()
        cold = _np(cold)
        a = args()
        warm = mpc.rollout_torch(*a, steps=steps, warm_start=True)
        torch.cuda.synchronize()
        final = a[0].cpu().numpy()
        warm = _np(warm)
        a2 = args()
        w2 = mpc.rollout_torch(*a2, steps=steps, warm_start=True, want_hist=False)      # a second call reuses the handle's buffer
        torch.cuda.synchronize()
        assert torch.equal(a2[0], a[0]) and np.array_equal(w2["status"].cpu().numpy(), warm["status"]) and np.array_equal(w2["iters"].cpu().numpy(), warm["iters"])
        st = mpc.stats()
    assert st.batch == B
    assert np.array_equal(final, warm["hist"][-1, :6])
    assert np.array_equal(warm["status"], cold["status"])                        # per car, the same worst status
    print("rollout B=1024, 6 steps: iterations cold %d, warm %d (%.3f)" % (cold["iters"].sum(), warm["iters"].sum(), warm["iters"].sum() / cold["iters"].sum()))
    assert warm["iters"].sum() < cold["iters"].sum()
    checked = 0
    for i in range(0, B, 32):
        s = list(sc["state"][:, i]); cfg.yaw_low, cfg.yaw_high = float(sc["yaw_lo"][i]), float(sc["yaw_hi"][i])
        oh = np.zeros((steps, 9)); worst = 0
        for t in range(steps):
            stt, o9, _, _, _ = O.mpc_solve(cfg, s, sc["coeffs"][:, i])
            oh[t] = o9; worst = max(worst, stt); s = list(o9[:6])
        assert (worst == 0) == (warm["status"][i] == 0)
        if worst != 0:
            continue
        checked += 1
        assert np.max(np.abs(warm["hist"][:, 6, i] - oh[:, 6])) < TOL_STEER
        assert np.max(np.abs(warm["hist"][:, 7, i] - oh[:, 7])) < TOL_ACCEL
        assert np.max(np.abs(warm["hist"][:, :6, i] - oh[:, :6])) < TOL_TRAJ
    assert checked >= 24


def test_in_place_buffers(pkg, golden_dir, waypoints, torch_dev):
    """warm_in is warm_out and warm_status is status: the results of separate buffers, bitwise -- on the wave kernel (192 instances)
    and on the lane kernel (the same 192 tiled to 8192: a launch with lane compaction), which also agree with each other bitwise."""
    import torch
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    cars = 192
    sc = pkg.scenarios.lake_track_batch(cars, params, waypoints, seed=7)
    got = {}
    for B in (8192, cars):
        idx = np.arange(B) % cars
        ins = [_t(sc["state"][:, idx], torch_dev), _t(sc["coeffs"][:, idx], torch_dev), _t(sc["yaw_lo"][idx], torch_dev), _t(sc["yaw_hi"][idx], torch_dev)]
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            first = mpc.solve_torch(*ins, want_warm=True)
            nxt = first["out"][:6].clone().contiguous()
            ins2 = [nxt] + ins[1:]
            sep = mpc.solve_torch(*ins2, warm=first["warm"].clone(), warm_status=first["status"].clone(), want_warm=True)
            torch.cuda.synchronize()
            sep = _np(sep)
            outputs = {"out": torch.empty_like(first["out"]), "status": first["status"], "iters": torch.empty_like(first["iters"]), "traj": None,
                       "warm": first["warm"]}
            inp = mpc.solve_torch(*ins2, warm=first["warm"], warm_status=first["status"], outputs=outputs)
            torch.cuda.synchronize()
            inp = _np(inp)
        for k in ("out", "status", "iters", "warm"):
            assert np.array_equal(sep[k], inp[k], equal_nan=True), (B, k)
        got[B] = sep
    for k in ("out", "status", "iters", "warm"):
        assert np.array_equal(got[8192][k][..., :cars], got[cars][k], equal_nan=True), k
        assert np.array_equal(got[8192][k][..., -cars:], got[cars][k][..., (np.arange(8192) % cars)[-cars:]], equal_nan=True), k


def _three_solves_ld16(pkg, params, b, B, dev):
    """On a fresh handle, through the C ABI with ld = ld_warm = 16 > B: the cold solve, the cold solve through the warm entry point
    (warm_in = NULL, warm_out given) and one warm solve started from that result in place (warm_in is warm_out, warm_status is
    status).  Every output array starts as a sentinel.  Returns the arrays of the three calls as numpy, all 16 columns."""
    import torch
    ld, F, I = 16, -7777.25, -12345
    rows = pkg.warm_rows(params.N)

    def inp(a):
        a = np.atleast_2d(np.asarray(a, dtype=np.float64))
        wide = np.zeros((a.shape[0], ld)); wide[:, :B] = a
        return _t(wide, dev)
    ff = lambda r: torch.full((r, ld), F, dtype=torch.float64, device=dev)
    ii = lambda: torch.full((ld,), I, dtype=torch.int32, device=dev)
    state, coeffs, ylo, yhi = inp(b["state"]), inp(b["coeffs"]), inp(b["yaw_lo"]), inp(b["yaw_hi"])
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    got = []

    def fetch(**k):
        torch.cuda.synchronize()
        got.append({n: v.cpu().numpy().copy() for n, v in k.items()})
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        out, traj, status, iters = ff(9), ff(2 * params.N), ii(), ii()
        assert lib.mpc_solve_batch_device(mpc._h, B, ld, state.data_ptr(), coeffs.data_ptr(), ylo.data_ptr(), yhi.data_ptr(), None, out.data_ptr(),
                                          traj.data_ptr(), status.data_ptr(), iters.data_ptr(), stream) == 0, lib.mpc_last_error()
        fetch(out=out, traj=traj, status=status, iters=iters)
        out, traj, status, iters, warm = ff(9), ff(2 * params.N), ii(), ii(), ff(rows)
        assert lib.mpc_solve_batch_device_warm(mpc._h, B, ld, state.data_ptr(), coeffs.data_ptr(), ylo.data_ptr(), yhi.data_ptr(), None, None, None,
                                               warm.data_ptr(), ld, None, out.data_ptr(), traj.data_ptr(), status.data_ptr(), iters.data_ptr(),
                                               stream) == 0, lib.mpc_last_error()
        fetch(out=out, traj=traj, status=status, iters=iters, warm=warm)
        nxt = out[:6].clone().contiguous()                       # (columns from B on are never read)
        out, traj, iters = ff(9), ff(2 * params.N), ii()
        assert lib.mpc_solve_batch_device_warm(mpc._h, B, ld, nxt.data_ptr(), coeffs.data_ptr(), ylo.data_ptr(), yhi.data_ptr(), None, warm.data_ptr(),
                                               status.data_ptr(), warm.data_ptr(), ld, None, out.data_ptr(), traj.data_ptr(), status.data_ptr(),
                                               iters.data_ptr(), stream) == 0, lib.mpc_last_error()
        fetch(out=out, traj=traj, status=status, iters=iters, warm=warm)
    return got, F, I


@pytest.mark.parametrize("lpi", [16, 32, 64])
def test_wave_groups_with_a_ragged_batch(pkg, golden_dir, waypoints, torch_dev, monkeypatch, lpi):
    """B = 7 with 16, 32 and 64 lanes per instance (MPC_WAVE_LPI overrides the whole-wave rule of small launches): the last wavefront of
    the 16- and 32-lane launches holds groups without an instance, and the warm wave kernel runs at every group size.  The cold solve,
    the cold solve through the warm entry point and a warm solve in place are BITWISE the lane kernel's in out, traj, status, iters and
    the warm buffer, and with ld = 16 nothing from column 7 on is written by either kernel."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    params.f64_f32_start = 0
    assert params.N == 10
    B = 7
    b = pkg.scenarios.lake_track_batch(B, params, waypoints, stream=3, filtered="survey")
    monkeypatch.setenv("MPC_WAVE_LPI", str(lpi))
    res = {}
    for mode, limit in (("lane", "0"), ("wave", "1024")):
        monkeypatch.setenv("MPC_WAVE_MAX_BATCH", limit)       # (read when the handle is created)
        res[mode], F, I = _three_solves_ld16(pkg, params, b, B, torch_dev)
    names = ("cold", "cold through the warm entry point", "warm in place")
    for name, lane, wave in zip(names, res["lane"], res["wave"]):
        assert sorted(lane) == sorted(wave) and ("warm" in lane) == (name != "cold")
        for k in lane:
            for mode, a in (("lane", lane[k]), ("wave", wave[k])):
                assert (a[..., B:] == (I if a.dtype == np.int32 else F)).all(), (lpi, name, mode, k, "written beyond column B - 1")
            assert np.array_equal(lane[k][..., :B], wave[k][..., :B], equal_nan=True), (lpi, name, k)
        assert (lane["status"][:B] != I).all() and (lane["iters"][:B] != I).all(), (lpi, name)
    # the warm entry point without a warm start is the cold solve, and the warm solve is another solve (it starts from the next state)
    cold, viaw, warm = res["wave"]
    for k in ("out", "traj", "status", "iters"):
        assert np.array_equal(cold[k], viaw[k], equal_nan=True), (lpi, k)
    assert not np.array_equal(warm["out"][:, :B], viaw["out"][:, :B])


def test_host_entry_point_and_fallbacks(pkg, warm_twin, golden_dir, waypoints, torch_dev):
    """mpc_solve_batch_host_warm: the device entry point's results; invalid columns and garbage end as the cold solve does."""
    from warm_helpers import garbage_warm
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    B = 256
    b = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=9)
    opts = pkg.warm_opts_default(shift=0)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        plain = mpc.solve_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"])
        cold = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], warm_opts=opts)
        for k in ("out", "status", "iters"):
            assert np.array_equal(plain[k], cold[k], equal_nan=True), k
        again = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], warm=cold["warm"], warm_status=cold["status"], warm_opts=opts)
        ok = cold["status"] == 0
        assert ok.mean() > 0.99 and np.array_equal(again["status"], cold["status"])
        assert (again["iters"][ok] < cold["iters"][ok]).all()
        assert np.abs(again["out"][6] - cold["out"][6])[ok].max() <= TOL_STEER and np.abs(again["out"][7] - cold["out"][7])[ok].max() <= TOL_ACCEL
        bad = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], warm=cold["warm"], warm_status=np.full(B, 2, np.int32), warm_opts=opts)
        for k in ("out", "status", "iters"):
            assert np.array_equal(bad[k], cold[k], equal_nan=True), k
        for name, g in zip(("nan", "far"), garbage_warm(params, cold["warm"])):
            r = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], warm=g, warm_opts=opts)
            assert np.array_equal(r["status"], cold["status"]), name
            assert np.isfinite(r["out"][:, ok]).all() and (r["iters"] >= cold["iters"]).all(), name
            assert np.abs(r["out"][6:8] - cold["out"][6:8])[:, ok].max() <= TOL_STEER and np.abs(r["out"][:6] - cold["out"][:6])[:, ok].max() <= TOL_TRAJ, name


def test_refusals(pkg, golden_dir, torch_dev):
    import torch
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    B = 64
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=torch_dev)
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device=torch_dev)
    lib = pkg.library()
    rows = pkg.warm_rows(params.N)

    def call(mpc, B, ld_warm, dtype=torch.float64):
        st, cf, yl, yh = (torch.zeros(s, dtype=dtype, device=torch_dev) for s in ((6, B), (5, B), (B,), (B,)))
        out, w, status, iters = torch.zeros((9, B), dtype=dtype, device=torch_dev), z(rows, max(B, 1)), zi(B), zi(B)
        return lib.mpc_solve_batch_device_warm(mpc._h, B, B, st.data_ptr(), cf.data_ptr(), yl.data_ptr(), yh.data_ptr(), None, None, None, w.data_ptr(),
                                               ld_warm, None, out.data_ptr(), None, status.data_ptr(), iters.data_ptr(), None)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        assert call(mpc, B, B) == 0
        torch.cuda.synchronize()
        assert call(mpc, B, B - 1) == -1 and b"ld_warm" in lib.mpc_last_error()
        assert call(mpc, 2 * B, 2 * B) == -1
        o = pkg.warm_opts_default(); o.size = 8
        st = z(6, B)
        assert lib.mpc_rollout_batch_device_warm(mpc._h, B, B, 2, st.data_ptr(), z(5, B).data_ptr(), z(B).data_ptr(), z(B).data_ptr(), None, C.byref(o), None,
                                                 zi(B).data_ptr(), None, None) == -1
    q = params.copy(); q.precision = pkg.PRECISION_F32
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        assert call(mpc, B, B, torch.float32) == -1
    q = params.copy(); q.max_soc = 4
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        assert call(mpc, B, B) == -4 and b"max_soc" in lib.mpc_last_error()
    q = params.copy(); q.f64_f32_start = 1
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        assert call(mpc, B, B) == -4 and b"f64_f32_start" in lib.mpc_last_error()
        with pytest.raises(pkg.MpcError):
            mpc.rollout_torch(z(6, B), z(5, B), z(B), z(B), steps=2, warm_start=True)


def test_drop_in_warm_start(pkg, golden_dir, tmp_path):
    exe = build_drop_in_warm(pkg, str(tmp_path))
    r = subprocess.run([exe, os.path.join(golden_dir, "config-stable.json"), "25"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = {"cold": [], "warm": []}; total = {}
    for l in r.stdout.strip().splitlines():
        p = l.split()
        if p[1] == "total":
            total[p[0]] = int(p[2])
        else:
            rows[p[0]].append([float(x) for x in p[2:]])
    cold, warm = np.array(rows["cold"]), np.array(rows["warm"])
    assert cold.shape == warm.shape == (25, 10)
    print("MPC::solve() x 25: iterations cold %d, warm %d" % (total["cold"], total["warm"]))
    assert np.abs(warm[:, 7] - cold[:, 7]).max() <= TOL_STEER and np.abs(warm[:, 8] - cold[:, 8]).max() <= TOL_ACCEL
    assert np.abs(warm[:, 1:7] - cold[:, 1:7]).max() <= TOL_TRAJ
    assert warm[0, 0] == cold[0, 0] and total["warm"] < total["cold"]
