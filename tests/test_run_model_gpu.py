"""run() and the telemetry handler with per-instance model values on the device (mpc_run_batch_device_model, mpc_telemetry_batch_device_model,
their _warm_model, _host_model and _host_warm_model forms, the two wire forms, run_torch / run_numpy / telemetry_torch with
``model``): the MODEL forms of the pre and post kernels around the wave kernels' MODEL builds (B <= wave_max_batch) or the lane
kernel's, against the oracle with a per-car OrcConfig, against the CPU build of the same functions (tests/host_twin, mpc_twin_run), and the two
paths against each other bit for bit.  N = 10, six waypoints per car."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ
from model_loop_helpers import steering_outside
from run_model_helpers import (EXTRA_LATENCY, FLEET_B, INFEASIBLE, NPTS, TOL_THROTTLE, assert_fleet_matches_oracle, assert_pre_matches_oracle, fleet, load_run_model_twin,
                               oracle_fleet, twin_run_model, uniform_model)
from run_warm_helpers import closed_loop

pytestmark = pytest.mark.gpu

CFG = "config-fast.json"
F, I = -7777.25, -12345          # what every output array holds before a call
KEYS = ("out8", "cmd", "status", "iters", "pre", "warm", "ptsx", "ptsy")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return load_run_model_twin()


@pytest.fixture(scope="module")
def fast(pkg, golden_dir):
    return pkg.params_from_json(os.path.join(golden_dir, CFG))


@pytest.fixture(scope="module")
def cars(pkg, fast, waypoints):
    """the stated population, and the next message of every car: its pose moved 0.3 m along its heading"""
    d = fleet(pkg, fast, waypoints)
    for k in ("pose", "tel"):
        nxt = d[k].copy()
        nxt[0] += 0.3 * np.cos(d[k][2]); nxt[1] += 0.3 * np.sin(d[k][2])
        d[k + "2"] = nxt
    return d


def _with(params, **kw):
    q = params.copy()
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _tiled(cars, B):
    """B cars: car j is car j % 48 of the population"""
    j = np.arange(B) % FLEET_B
    return {k: np.ascontiguousarray(v[:, j]) for k, v in cars.items()}


def _call(pkg, mpc, dev, rows, ptsx, ptsy, model, tel=False, ld=None, rec=None, warm=False, opts=None, plain=False):
    """One device call through the C ABI with leading dimension ld >= B and ld_warm = ld + 8, every output a sentinel first.
    rec = None: the entry point without warm arguments (_model, or with plain=True / model=None the one without _model); rec = {}:
    the _warm_model form with warm_in = NULL, its record and status kept in `rec`; warm = True: from the record in `rec`, in place.
    -> numpy arrays cut to B columns, "pad": nothing from column B on was written."""
    import torch
    B = rows.shape[1]
    ld = B if ld is None else ld
    ldw = ld + 8
    lib = pkg.library()

    def inp(a):
        wide = np.zeros((a.shape[0], ld)); wide[:, :B] = a
        return torch.from_numpy(wide).to(dev)
    ff = lambda r, l=ld: torch.full((r, l), F, dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    t_rows, px, py = inp(rows), inp(ptsx), inp(ptsy)
    md = inp(model) if model is not None else None
    out8, cmd, pre = ff(8), ff(2), ff(15)
    iters = torch.full((ld,), I, dtype=torch.int32, device=dev)
    if rec is not None and not warm:
        rec["warm"] = ff(mpc.warm_rows(), ldw); rec["status"] = torch.full((ld,), I, dtype=torch.int32, device=dev)
    status = rec["status"] if rec is not None else torch.full((ld,), I, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    h = mpc._h
    o = C.byref(opts) if opts is not None else None
    if rec is None:
        if tel and plain:
            rc = lib.mpc_telemetry_batch_device(h, B, ld, NPTS, p(t_rows), EXTRA_LATENCY, p(px), p(py), p(cmd), p(out8), p(status), stream)
        elif tel:
            rc = lib.mpc_telemetry_batch_device_model(h, B, ld, NPTS, p(t_rows), EXTRA_LATENCY, p(px), p(py), p(md), p(cmd), p(out8), p(status), stream)
        elif plain:
            rc = lib.mpc_run_batch_device(h, B, ld, NPTS, p(t_rows), p(px), p(py), p(out8), None, p(status), p(iters), p(pre), stream)
        else:
            rc = lib.mpc_run_batch_device_model(h, B, ld, NPTS, p(t_rows), p(px), p(py), p(md), p(out8), None, p(status), p(iters), p(pre), stream)
    else:
        w_in, w_st = (p(rec["warm"]), p(rec["status"])) if warm else (None, None)
        wargs = (w_in, w_st, p(rec["warm"]), ldw, o)
        if tel and plain:
            rc = lib.mpc_telemetry_batch_device_warm(h, B, ld, NPTS, p(t_rows), EXTRA_LATENCY, p(px), p(py), *wargs, p(cmd), p(out8), p(status), stream)
        elif tel:
            rc = lib.mpc_telemetry_batch_device_warm_model(h, B, ld, NPTS, p(t_rows), EXTRA_LATENCY, p(px), p(py), p(md), *wargs, p(cmd), p(out8), p(status), stream)
        elif plain:
            rc = lib.mpc_run_batch_device_warm(h, B, ld, NPTS, p(t_rows), p(px), p(py), *wargs, p(out8), None, p(status), p(iters), p(pre), stream)
        else:
            rc = lib.mpc_run_batch_device_warm_model(h, B, ld, NPTS, p(t_rows), p(px), p(py), p(md), *wargs, p(out8), None, p(status), p(iters), p(pre), stream)
    torch.cuda.synchronize()
    if rc != 0:
        return {"rc": rc, "msg": lib.mpc_last_error()}
    n = lambda t: t.cpu().numpy()
    res = {"rc": 0, "out8": n(out8), "cmd": n(cmd), "status": n(status), "iters": n(iters), "pre": n(pre), "ptsx": n(px), "ptsy": n(py),
           "warm": n(rec["warm"]) if rec is not None else None}
    pad = True
    for k in ("out8", "cmd", "status", "iters", "pre", "warm"):
        if res[k] is not None:
            pad = pad and bool((res[k][..., B:] == (I if res[k].dtype == np.int32 else F)).all())
            res[k] = np.ascontiguousarray(res[k][..., :B])
    res["ptsx"] = res["ptsx"][:, :B]; res["ptsy"] = res["ptsy"][:, :B]
    res["pad"] = pad
    if tel:           # (the telemetry forms return neither iterations nor pre)
        res["iters"] = res["pre"] = None
    else:
        res["cmd"] = None
    return res


def _sequence(pkg, params, d, dev, ld=None, max_batch=None, model=None):
    """On a fresh handle, for the cars of `d`: run() cold, run() through the warm form with warm_in = NULL, the next message warm in
    place; then the same three for the telemetry handler.  -> the six results."""
    B = d["pose"].shape[1]
    model = d["model"] if model is None else model
    out = []
    with pkg.BatchedMPC(params, max_batch or B, device=0) as mpc:
        for tel, rows, rows2 in ((False, d["pose"], d["pose2"]), (True, d["tel"], d["tel2"])):
            rec = {}
            out.append(_call(pkg, mpc, dev, rows, d["ptsx"], d["ptsy"], model, tel=tel, ld=ld))
            out.append(_call(pkg, mpc, dev, rows, d["ptsx"], d["ptsy"], model, tel=tel, ld=ld, rec=rec))
            out.append(_call(pkg, mpc, dev, rows2, d["ptsx"], d["ptsy"], model, tel=tel, ld=ld, rec=rec, warm=True))
    for r in out:
        assert r["rc"] == 0, r.get("msg")
        assert r["pad"], "written beyond column B - 1"
    return out


NAMES = ("run cold", "run cold through the warm form", "run warm in place", "telemetry cold", "telemetry cold through the warm form",
         "telemetry warm in place")


def _assert_bitwise(a, b, what, cols=None):
    for name, x, y in zip(NAMES, a, b):
        for k in KEYS:
            if x[k] is None:
                assert y[k] is None
                continue
            yy = y[k] if cols is None else y[k][..., cols]
            assert np.array_equal(x[k], yy, equal_nan=True), (what, name, k)


@pytest.fixture(scope="module")
def wave48(pkg, fast, cars, torch_dev):
    """test 1's calls: B = 48 on a default handle (the wave path), ld = 64"""
    return _sequence(pkg, fast, cars, torch_dev, ld=64)


@pytest.fixture(scope="module")
def lane48(pkg, fast, cars, torch_dev):
    """the same calls on a handle that never takes the wave path"""
    return _sequence(pkg, _with(fast, wave_max_batch=-1), cars, torch_dev, ld=64)


@pytest.fixture(scope="module")
def oracle48(cars):
    return {"run": oracle_fleet(CFG, cars["pose"], cars["ptsx"], cars["ptsy"], cars["model"]),
            "run2": oracle_fleet(CFG, cars["pose2"], cars["ptsx"], cars["ptsy"], cars["model"]),
            "tel": oracle_fleet(CFG, cars["tel"], cars["ptsx"], cars["ptsy"], cars["model"], tel=True, extra=EXTRA_LATENCY),
            "tel2": oracle_fleet(CFG, cars["tel2"], cars["ptsx"], cars["ptsy"], cars["model"], tel=True, extra=EXTRA_LATENCY)}


def _assert_follows_twin(g, tw, model, what):
    """device against the CPU build of the same header (the reciprocals, sin / cos and the FMA contraction differ, so the bits do not
    carry over): the same status everywhere, and where the iteration counts agree the outputs agree within the tolerances"""
    assert np.array_equal(g["status"], tw["status"]), (what, np.where(g["status"] != tw["status"])[0][:8])
    both = (g["status"] == 0) & (g["iters"] == tw["iters"])
    print("%s vs CPU build: %d of %d with the same iteration count" % (what, int(both.sum()), both.size))
    assert both.any(), what
    d = np.abs(g["out8"] - tw["out8"])[:, both]
    assert (d[4] * model[2, both]).max() <= TOL_STEER and d[5].max() <= TOL_ACCEL and np.delete(d, (4, 5), axis=0).max() <= TOL_TRAJ, what


def test_oracle_parity_on_the_wave_path(pkg, fast, cars, twin, wave48, oracle48):
    """B = 48 <= wave_max_batch on a default handle: the MODEL builds of the two wave kernels between the MODEL pre and post kernels.
    run() with ld = 64 and the telemetry handler, cold and warm, against the oracle with a Config per car; run() against the CPU
    build; `pre` and the vehicle-frame waypoints against what the oracle's run() derives."""
    model = cars["model"]
    run_cold, run_viaw, run_warm, tel_cold, tel_viaw, tel_warm = wave48
    assert_fleet_matches_oracle(run_cold, oracle48["run"], model, what="run(), wave, cold")
    assert_fleet_matches_oracle(run_warm, oracle48["run2"], model, what="run(), wave, warm")
    assert_fleet_matches_oracle(tel_cold, oracle48["tel"], model, tel=True, what="telemetry, wave, cold")
    assert_fleet_matches_oracle(tel_warm, oracle48["tel2"], model, tel=True, what="telemetry, wave, warm")
    assert_pre_matches_oracle(run_cold, oracle48["run"], what="run(), wave")
    assert (oracle48["run"]["status"] == INFEASIBLE).sum() == 4
    opts = pkg.warm_opts_default()
    t1 = twin_run_model(twin, fast, cars["pose"], cars["ptsx"], cars["ptsy"], model, opts)
    _assert_follows_twin(run_cold, t1, model, "run(), wave, cold")
    assert np.abs(run_cold["pre"] - t1["pre"]).max() <= 1e-9
    t2 = twin_run_model(twin, fast, cars["pose2"], cars["ptsx"], cars["ptsy"], model, opts, warm=t1["warm"], warm_status=t1["status"])
    _assert_follows_twin(run_warm, t2, model, "run(), wave, warm")
    # the telemetry handler against the CPU build: the entry point returns no iteration counts, so every car both converge on is
    # compared (both end at the same KKT point to the solver's tolerance, as against the oracle)
    u1 = twin_run_model(twin, fast, cars["tel"], cars["ptsx"], cars["ptsy"], model, opts, tel=True, extra=EXTRA_LATENCY)
    u2 = twin_run_model(twin, fast, cars["tel2"], cars["ptsx"], cars["ptsy"], model, opts, tel=True, extra=EXTRA_LATENCY, warm=u1["warm"], warm_status=u1["status"])
    for g, tw, what in ((tel_cold, u1, "cold"), (tel_warm, u2, "warm")):
        assert np.array_equal(g["status"], tw["status"]), what
        both = g["status"] == 0
        assert both.any(), what
        d = np.abs(g["out8"] - tw["out8"])[:, both]; c = np.abs(g["cmd"] - tw["cmd"])[:, both]
        print("telemetry, wave, %s vs CPU build: %d cars, max |d steer| %.3g rad, |d accel| %.3g, |d other| %.3g, |d throttle| %.3g" % (
            what, int(both.sum()), (d[4] * model[2, both]).max(), d[5].max(), np.delete(d, (4, 5), axis=0).max(), c[1].max()))
        assert (d[4] * model[2, both]).max() <= TOL_STEER and d[5].max() <= TOL_ACCEL and np.delete(d, (4, 5), axis=0).max() <= TOL_TRAJ, what
        assert (c[0] * model[2, both]).max() <= TOL_STEER and c[1].max() <= TOL_THROTTLE, what
    # warm_in = NULL is the cold call, and the warm call needs fewer iterations
    for k in ("out8", "status", "iters", "pre", "ptsx"):
        assert np.array_equal(run_cold[k], run_viaw[k], equal_nan=True), k
    assert np.array_equal(tel_cold["cmd"], tel_viaw["cmd"]) and np.array_equal(tel_cold["status"], tel_viaw["status"])
    assert run_warm["iters"].sum() < run_cold["iters"].sum()
    assert np.isfinite(run_viaw["warm"]).all() and np.isfinite(run_warm["warm"]).all()


@pytest.mark.parametrize("B", [48, 1, 5, 18])
def test_wave_is_lane_bitwise(pkg, fast, cars, torch_dev, wave48, lane48, B):
    """The wave kernels' MODEL builds write what the lane kernel's write: out8, cmd, status, iters, pre and warm_out, cold and warm.
    B = 1 and B = 5: launches up to 16 cars give every car a whole wave (64 lanes per instance, a grid of B).  B = 48: four cars per
    wavefront, every wavefront full.  B = 18: four full wavefronts and one that holds two cars -- the lanes of its other two groups
    leave at once."""
    if B == 48:
        _assert_bitwise(wave48, lane48, "B = 48")
        return
    d = {k: np.ascontiguousarray(v[:, 3:3 + B]) for k, v in cars.items()}
    wave = _sequence(pkg, fast, d, torch_dev, ld=24)
    lane = _sequence(pkg, _with(fast, wave_max_batch=-1), d, torch_dev, ld=24)
    _assert_bitwise(wave, lane, "B = %d" % B)
    _assert_bitwise(wave, lane48, "B = %d against B = 48" % B, cols=slice(3, 3 + B))


def test_wave_groups_of_32_lanes(pkg, fast, cars, torch_dev, lane48, monkeypatch):
    """B = 48 is above the size that gets a whole wave per car: 16 lanes per car by default.  The 32-lane groups as well: 24 full
    wavefronts at B = 48, and at B = 19 a last wavefront that holds one car."""
    monkeypatch.setenv("MPC_WAVE_LPI", "32")
    _assert_bitwise(_sequence(pkg, fast, cars, torch_dev, ld=64), lane48, "32 lanes per car")
    d = {k: np.ascontiguousarray(v[:, :19]) for k, v in cars.items()}
    _assert_bitwise(_sequence(pkg, fast, d, torch_dev, ld=24), lane48, "32 lanes per car, B = 19", cols=slice(0, 19))


def test_above_the_wave_limit(pkg, fast, cars, torch_dev, lane48):
    """B = 1 100 > wave_max_batch on a default handle (ld = 1 152): the lane kernel's MODEL build, column j bitwise column j % 48 of
    the B = 48 lane call.  B = 8 256: lane compaction moves instances, their columns follow -- bitwise lane_compact = 0."""
    j = np.arange(1100) % FLEET_B
    _assert_bitwise(_sequence(pkg, fast, _tiled(cars, 1100), torch_dev, ld=1152), lane48, "B = 1100", cols=j)
    big = _tiled(cars, 8256)
    on = _sequence(pkg, fast, big, torch_dev)
    off = _sequence(pkg, _with(fast, lane_compact=0), big, torch_dev)
    _assert_bitwise(on, off, "B = 8256, lane compaction")
    _assert_bitwise(on, lane48, "B = 8256", cols=np.arange(8256) % FLEET_B)


def test_warm_handler_loop(pkg, fast, cars, waypoints, torch_dev):
    """Six messages per car, each car moved by the ideal plant with its own max_steering; message 1 cold, the others warm in place
    (warm_in == warm_out, warm_status == status).  Every solve: the oracle's cold status and its outputs within the tolerances.
    The warm solves take fewer iterations than cold model calls on the same messages."""
    import torch
    steps, model = 6, cars["model"]
    sc = pkg.scenarios.lake_track_batch(FLEET_B, fast, waypoints, seed=77)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dev)
    md = t(model)
    with pkg.BatchedMPC(fast, FLEET_B, device=0) as mpc:
        warm = torch.empty((mpc.warm_rows(), FLEET_B), dtype=torch.float64, device=torch_dev)
        status = torch.empty((FLEET_B,), dtype=torch.int32, device=torch_dev)

        def step(k, pose, px, py):
            r = mpc.run_torch(t(pose), t(px), t(py), warm=warm if k > 0 else None, warm_status=status if k > 0 else None, warm_out=warm,
                              status_out=status, model=md)
            torch.cuda.synchronize()
            assert r["warm"] is warm and r["status"] is status
            return {k_: r[k_].cpu().numpy() for k_ in ("out8", "status", "iters")}
        rec = closed_loop(step, sc, waypoints, steps, model[2])
        cold_iters = 0
        for k in range(1, steps):
            c = mpc.run_torch(t(rec["pose"][k]), t(rec["ptsx"][k]), t(rec["ptsy"][k]), model=md)
            torch.cuda.synchronize()
            cold_iters += int(c["iters"].sum().item())
    for k in range(steps):
        ref = oracle_fleet(CFG, rec["pose"][k], rec["ptsx"][k], rec["ptsy"][k], model)
        got = {"out8": rec["out8"][k], "status": rec["status"][k]}
        # (a car the oracle refuses is reported with the start point and stands still: from then on its limit holds)
        assert_fleet_matches_oracle(got, ref, model, what="message %d" % (k + 1), min_converged=40)
    warm_iters = int(rec["iters"][1:].sum())
    print("handler loop, messages 2..%d: warm %d iterations, cold %d, ratio %.3f" % (steps, warm_iters, cold_iters, warm_iters / cold_iters))
    assert warm_iters < cold_iters


@pytest.mark.parametrize("wave_max_batch", [0, -1])
def test_a_record_from_a_wider_column_starts_cold(pkg, fast, cars, torch_dev, wave_max_batch):
    """Records written under one column and handed to a column with a narrower max_steering that they violate: those cars are bitwise
    the cold model call, iterations included; the others start warm.  On the wave path and on the lane path."""
    model = cars["model"]
    with pkg.BatchedMPC(_with(fast, wave_max_batch=wave_max_batch), FLEET_B, device=0) as mpc:
        rec = {}
        first = _call(pkg, mpc, torch_dev, cars["pose"], cars["ptsx"], cars["ptsy"], model, rec=rec)
        peak = np.abs(first["warm"].reshape(fast.N - 1, 22, -1)[:, 6, :]).max(0)
        narrow = model.copy()
        pick = np.where((first["status"] == 0) & (peak > 0.02))[0][::2]
        narrow[2, pick] = 0.5 * peak[pick]
        out = steering_outside(fast.N, first["warm"], narrow[2]) & (first["status"] == 0)
        assert np.array_equal(np.where(out)[0], pick) and len(pick) >= 8
        cold = _call(pkg, mpc, torch_dev, cars["pose2"], cars["ptsx"], cars["ptsy"], narrow)
        warm = _call(pkg, mpc, torch_dev, cars["pose2"], cars["ptsx"], cars["ptsy"], narrow, rec=rec, warm=True)
    for k in ("out8", "status", "iters", "pre"):
        assert np.array_equal(warm[k][..., out], cold[k][..., out]), k
    rest = ~out & (first["status"] == 0) & (cold["status"] == 0)
    assert warm["iters"][rest].sum() < cold["iters"][rest].sum()


@pytest.mark.parametrize("wave_max_batch", [0, -1])
def test_max_soc_cold(pkg, fast, golden_dir, waypoints, torch_dev, wave_max_batch):
    """max_soc = 4 with uniform columns on the hard N = 10 instances of tests/golden/soc_instances.npz, fed as the poses and waypoints
    they were made from (its provenance: lake_track_batch(65 536, stream 3, filtered 'survey'), rows n10_index -- run_pre gives the
    fixture's states and coefficients back): status and iterations are those of the plain run call on the same handle, on the wave
    path (B = 178) and on the lane path."""
    z = np.load(os.path.join(golden_dir, "soc_instances.npz"))
    idx = z["n10_index"]
    pop = pkg.scenarios.lake_track_batch(65536, fast, waypoints, stream=3, filtered="survey")
    assert np.array_equal(pop["state"][:, idx], z["n10_state"])
    d = {k: np.ascontiguousarray(pop[k][:, idx], dtype=np.float64) for k in ("pose", "ptsx", "ptsy")}
    B = len(idx)
    p4 = _with(fast, max_soc=4, wave_max_batch=wave_max_batch)
    with pkg.BatchedMPC(p4, B, device=0) as mpc:
        plain = _call(pkg, mpc, torch_dev, d["pose"], d["ptsx"], d["ptsy"], None, plain=True)
        got = _call(pkg, mpc, torch_dev, d["pose"], d["ptsx"], d["ptsy"], uniform_model(p4, B))
    with pkg.BatchedMPC(_with(p4, max_soc=0), B, device=0) as mpc:
        soc0 = _call(pkg, mpc, torch_dev, d["pose"], d["ptsx"], d["ptsy"], uniform_model(p4, B))
    for k in ("status", "iters", "out8", "pre"):
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    assert got["iters"].sum() < soc0["iters"].sum()           # the correction is at work


def _host_args(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def test_model_null_is_the_entry_point_without_model(pkg, fast, cars, torch_dev):
    """model = NULL: all eight forms and the two wire forms are bitwise the entry points without _model"""
    lib = pkg.library()
    B = 7
    d = {k: np.ascontiguousarray(v[:, :B]) for k, v in cars.items()}
    v = _host_args
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        # the four device forms
        for tel in (False, True):
            rows, rows2 = (d["tel"], d["tel2"]) if tel else (d["pose"], d["pose2"])
            ra, rb = {}, {}
            a = [_call(pkg, mpc, torch_dev, rows, d["ptsx"], d["ptsy"], None, tel=tel, ld=8, plain=True),
                 _call(pkg, mpc, torch_dev, rows, d["ptsx"], d["ptsy"], None, tel=tel, ld=8, plain=True, rec=ra),
                 _call(pkg, mpc, torch_dev, rows2, d["ptsx"], d["ptsy"], None, tel=tel, ld=8, plain=True, rec=ra, warm=True)]
            b = [_call(pkg, mpc, torch_dev, rows, d["ptsx"], d["ptsy"], None, tel=tel, ld=8),
                 _call(pkg, mpc, torch_dev, rows, d["ptsx"], d["ptsy"], None, tel=tel, ld=8, rec=rb),
                 _call(pkg, mpc, torch_dev, rows2, d["ptsx"], d["ptsy"], None, tel=tel, ld=8, rec=rb, warm=True)]
            for x, y in zip(a, b):
                assert x["rc"] == 0 and y["rc"] == 0 and x["pad"] and y["pad"]
                for k in KEYS:
                    assert (x[k] is None and y[k] is None) or np.array_equal(x[k], y[k], equal_nan=True), (tel, k)
        # the four host forms and the two wire forms
        rows_w = mpc.warm_rows()

        def host_run(fn, extra_args, warm_args):
            px, py = d["ptsx"].copy(), d["ptsy"].copy()
            o8 = np.zeros((8, B)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32); pre = np.zeros((15, B))
            assert fn(mpc._h, B, B, NPTS, v(d["pose"]), v(px), v(py), *extra_args, *warm_args, v(o8), None, v(st), v(it), v(pre)) == 0, lib.mpc_last_error()
            return [o8, st, it, pre, px, py]

        def host_tel(fn, extra_args, warm_args):
            cmd = np.zeros((2, B)); st = np.zeros(B, dtype=np.int32)
            assert fn(mpc._h, B, B, NPTS, v(d["tel"]), EXTRA_LATENCY, v(d["ptsx"]), v(d["ptsy"]), *extra_args, *warm_args, v(cmd), v(st)) == 0, lib.mpc_last_error()
            return [cmd, st]
        W = (pkg.MpcWireTelemetry * B)()
        for i in range(B):
            W[i].x, W[i].y, W[i].psi, W[i].speed, W[i].steering_angle, W[i].throttle, W[i].npts = *d["tel"][:5, i], 0.0, NPTS
            for q in range(NPTS):
                W[i].ptsx[q] = d["ptsx"][q, i]; W[i].ptsy[q] = d["ptsy"][q, i]
        prev = np.ascontiguousarray(d["tel"][5])

        def wire(fn, extra_args, warm_args):
            cmd = np.zeros((2, B)); st = np.zeros(B, dtype=np.int32)
            assert fn(mpc._h, B, W, v(prev), EXTRA_LATENCY, *extra_args, *warm_args, v(cmd), v(st)) == 0, lib.mpc_last_error()
            return [cmd, st]
        for run, plain_fn, model_fn, plain_w, model_w in ((host_run, lib.mpc_run_batch_host, lib.mpc_run_batch_host_model, lib.mpc_run_batch_host_warm,
                                                           lib.mpc_run_batch_host_warm_model),
                                                          (host_tel, lib.mpc_telemetry_batch_host, lib.mpc_telemetry_batch_host_model,
                                                           lib.mpc_telemetry_batch_host_warm, lib.mpc_telemetry_batch_host_warm_model),
                                                          (wire, lib.mpc_wire_telemetry_batch_host, lib.mpc_wire_telemetry_batch_host_model,
                                                           lib.mpc_wire_telemetry_batch_host_warm, lib.mpc_wire_telemetry_batch_host_warm_model)):
            for x, y in zip(run(plain_fn, (), ()), run(model_fn, (None,), ())):
                assert np.array_equal(x, y, equal_nan=True)
            wa, wb = np.zeros((rows_w, B)), np.zeros((rows_w, B))
            for x, y in zip(run(plain_w, (), (None, None, v(wa), B, None)), run(model_w, (None,), (None, None, v(wb), B, None))):
                assert np.array_equal(x, y, equal_nan=True)
            assert np.array_equal(wa, wb, equal_nan=True) and np.abs(wa).max() > 0


def test_refusals_and_accepted_handles(pkg, fast, golden_dir, cars, torch_dev):
    B = 16
    d = {k: np.ascontiguousarray(v[:, :B]) for k, v in cars.items()}
    lib = pkg.library()
    args = (d["pose"], d["ptsx"], d["ptsy"], d["model"])
    # an MPC_PRECISION_F32 handle: MPC_ERR_INVALID with the model message, cold and warm, run() and telemetry
    with pkg.BatchedMPC(_with(fast, precision=pkg.PRECISION_F32), B, device=0) as mpc:
        for tel in (False, True):
            for rec in (None, {}):
                r = _call(pkg, mpc, torch_dev, *args, tel=tel, rec=rec)
                assert r["rc"] == -1 and b"per-instance model values" in r["msg"], r
    # warm with max_soc = 4: MPC_ERR_UNSUPPORTED; the cold forms are served
    with pkg.BatchedMPC(_with(fast, max_soc=4), B, device=0) as mpc:
        for tel in (False, True):
            r = _call(pkg, mpc, torch_dev, *args, tel=tel, rec={})
            assert r["rc"] == -4 and b"max_soc" in r["msg"], r
            assert _call(pkg, mpc, torch_dev, *args, tel=tel)["rc"] == 0
    # ld_warm < B and npts = 2: MPC_ERR_INVALID
    import torch
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_dev)
        pose, px, py, md = (t(a) for a in args)
        o8 = torch.zeros((8, B), dtype=torch.float64, device=torch_dev); st = torch.zeros(B, dtype=torch.int32, device=torch_dev)
        w = torch.zeros((mpc.warm_rows(), B), dtype=torch.float64, device=torch_dev)
        p = lambda x: x.data_ptr()
        assert lib.mpc_run_batch_device_warm_model(mpc._h, B, B, NPTS, p(pose), p(px), p(py), p(md), None, None, p(w), B - 1, None, p(o8), None, p(st), None,
                                                   None, None) == -1
        assert b"ld_warm" in lib.mpc_last_error()
        assert lib.mpc_run_batch_device_model(mpc._h, B, B, 2, p(pose), p(px), p(py), p(md), p(o8), None, p(st), None, None, None) == -1
        assert b"npts" in lib.mpc_last_error()
        torch.cuda.synchronize()
    # an N = 25 handle as created by default (its ordinary solve starts in fp32) is served, cold and warm, bitwise a handle with
    # f64_f32_start = 0 -- on the wave path (B = 16) and above it (B = 1 100)
    n25 = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"), N=25, dt=0.05)
    for Bn in (B, 1100):
        dn = _tiled(cars, Bn)
        a = _sequence(pkg, n25, dn, torch_dev)
        b = _sequence(pkg, _with(n25, f64_f32_start=0), dn, torch_dev)
        _assert_bitwise(a, b, "N = 25, B = %d" % Bn)
        assert (a[0]["status"] == 0).sum() >= 0.8 * Bn


def test_host_and_python_forms(pkg, fast, cars, torch_dev):
    """_host_model and _host_warm_model are bitwise the device forms at B = 7; run_numpy(model=...), telemetry_torch(model=...) and the
    wire form at B = 3 are mpc_telemetry_batch_host_model / mpc_run_batch_host_model."""
    import torch
    lib = pkg.library()
    v = _host_args
    B = 7
    d = {k: np.ascontiguousarray(v_[:, :B]) for k, v_ in cars.items()}
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        dev = _sequence_on(pkg, mpc, d, torch_dev)
        rows_w = mpc.warm_rows()
        # run(): cold, cold through the warm form, warm from that record
        px, py = d["ptsx"].copy(), d["ptsy"].copy()
        o8 = np.zeros((8, B)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32); pre = np.zeros((15, B))
        assert lib.mpc_run_batch_host_model(mpc._h, B, B, NPTS, v(d["pose"]), v(px), v(py), v(d["model"]), v(o8), None, v(st), v(it), v(pre)) == 0, lib.mpc_last_error()
        for k, a in (("out8", o8), ("status", st), ("iters", it), ("pre", pre), ("ptsx", px), ("ptsy", py)):
            assert np.array_equal(a, dev[0][k], equal_nan=True), k
        w = np.zeros((rows_w, B)); px, py = d["ptsx"].copy(), d["ptsy"].copy()
        assert lib.mpc_run_batch_host_warm_model(mpc._h, B, B, NPTS, v(d["pose"]), v(px), v(py), v(d["model"]), None, None, v(w), B, None, v(o8), None, v(st),
                                                 v(it), v(pre)) == 0, lib.mpc_last_error()
        assert np.array_equal(w, dev[1]["warm"], equal_nan=True) and np.array_equal(o8, dev[1]["out8"], equal_nan=True)
        px, py = d["ptsx"].copy(), d["ptsy"].copy()
        assert lib.mpc_run_batch_host_warm_model(mpc._h, B, B, NPTS, v(d["pose2"]), v(px), v(py), v(d["model"]), v(w), v(st), v(w), B, None, v(o8), None, v(st),
                                                 v(it), v(pre)) == 0, lib.mpc_last_error()
        for k, a in (("out8", o8), ("status", st), ("iters", it), ("pre", pre), ("warm", w)):
            assert np.array_equal(a, dev[2][k], equal_nan=True), k
        # the telemetry handler likewise
        cmd = np.zeros((2, B)); st = np.zeros(B, dtype=np.int32)
        assert lib.mpc_telemetry_batch_host_model(mpc._h, B, B, NPTS, v(d["tel"]), EXTRA_LATENCY, v(d["ptsx"]), v(d["ptsy"]), v(d["model"]), v(cmd), v(st)) == 0
        assert np.array_equal(cmd, dev[3]["cmd"]) and np.array_equal(st, dev[3]["status"])
        w = np.zeros((rows_w, B))
        assert lib.mpc_telemetry_batch_host_warm_model(mpc._h, B, B, NPTS, v(d["tel"]), EXTRA_LATENCY, v(d["ptsx"]), v(d["ptsy"]), v(d["model"]), None, None,
                                                       v(w), B, None, v(cmd), v(st)) == 0
        assert np.array_equal(w, dev[4]["warm"], equal_nan=True) and np.array_equal(cmd, dev[4]["cmd"])
        assert lib.mpc_telemetry_batch_host_warm_model(mpc._h, B, B, NPTS, v(d["tel2"]), EXTRA_LATENCY, v(d["ptsx"]), v(d["ptsy"]), v(d["model"]), v(w), v(st),
                                                       v(w), B, None, v(cmd), v(st)) == 0
        assert np.array_equal(cmd, dev[5]["cmd"]) and np.array_equal(st, dev[5]["status"]) and np.array_equal(w, dev[5]["warm"], equal_nan=True)
    # Python and the wire form at B = 3
    B = 3
    d = {k: np.ascontiguousarray(v_[:, :B]) for k, v_ in cars.items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dev)
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        cmd = np.zeros((2, B)); st = np.zeros(B, dtype=np.int32)
        assert lib.mpc_telemetry_batch_host_model(mpc._h, B, B, NPTS, v(d["tel"]), EXTRA_LATENCY, v(d["ptsx"]), v(d["ptsy"]), v(d["model"]), v(cmd), v(st)) == 0
        r = mpc.telemetry_torch(t(d["tel"]), t(d["ptsx"]), t(d["ptsy"]), extra_latency=EXTRA_LATENCY, model=t(d["model"]))
        torch.cuda.synchronize()
        assert np.array_equal(r["cmd"].cpu().numpy(), cmd) and np.array_equal(r["status"].cpu().numpy(), st)
        W = (pkg.MpcWireTelemetry * B)()
        for i in range(B):
            W[i].x, W[i].y, W[i].psi, W[i].speed, W[i].steering_angle, W[i].throttle, W[i].npts = *d["tel"][:5, i], 0.0, NPTS
            for q in range(NPTS):
                W[i].ptsx[q] = d["ptsx"][q, i]; W[i].ptsy[q] = d["ptsy"][q, i]
        prev = np.ascontiguousarray(d["tel"][5])
        wcmd = np.zeros((2, B)); wst = np.zeros(B, dtype=np.int32)
        assert lib.mpc_wire_telemetry_batch_host_model(mpc._h, B, W, v(prev), EXTRA_LATENCY, v(d["model"]), v(wcmd), v(wst)) == 0, lib.mpc_last_error()
        assert np.array_equal(wcmd, cmd) and np.array_equal(wst, st)
        ww = np.zeros((mpc.warm_rows(), B))
        assert lib.mpc_wire_telemetry_batch_host_warm_model(mpc._h, B, W, v(prev), EXTRA_LATENCY, v(d["model"]), None, None, v(ww), B, None, v(wcmd), v(wst)) == 0
        assert np.array_equal(wcmd, cmd) and np.isfinite(ww).all() and np.abs(ww).max() > 0
        # run_numpy / run_torch against mpc_run_batch_host_model
        px, py = d["ptsx"].copy(), d["ptsy"].copy()
        o8 = np.zeros((8, B)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32); pre = np.zeros((15, B))
        assert lib.mpc_run_batch_host_model(mpc._h, B, B, NPTS, v(d["pose"]), v(px), v(py), v(d["model"]), v(o8), None, v(st), v(it), v(pre)) == 0
        rn = mpc.run_numpy(d["pose"], d["ptsx"], d["ptsy"], model=d["model"])
        rt = mpc.run_torch(t(d["pose"]), t(d["ptsx"]), t(d["ptsy"]), want_pre=True, model=t(d["model"]))
        torch.cuda.synchronize()
        for k, a in (("out8", o8), ("status", st), ("iters", it), ("pre", pre)):
            assert np.array_equal(rn[k], a, equal_nan=True) and np.array_equal(rt[k].cpu().numpy(), a, equal_nan=True), k
        rw = mpc.run_numpy(d["pose2"], d["ptsx"], d["ptsy"], model=d["model"], warm=mpc.run_numpy(d["pose"], d["ptsx"], d["ptsy"], model=d["model"], want_warm=True)["warm"],
                           warm_status=st)
        assert rw["iters"].sum() < it.sum() and np.array_equal(rw["status"], st)
        with pytest.raises(ValueError):
            mpc.run_numpy(d["pose"], d["ptsx"], d["ptsy"], model=d["model"][:5])


def _sequence_on(pkg, mpc, d, dev):
    """_sequence on an open handle"""
    out = []
    for tel, rows, rows2 in ((False, d["pose"], d["pose2"]), (True, d["tel"], d["tel2"])):
        rec = {}
        out.append(_call(pkg, mpc, dev, rows, d["ptsx"], d["ptsy"], d["model"], tel=tel))
        out.append(_call(pkg, mpc, dev, rows, d["ptsx"], d["ptsy"], d["model"], tel=tel, rec=rec))
        out.append(_call(pkg, mpc, dev, rows2, d["ptsx"], d["ptsy"], d["model"], tel=tel, rec=rec, warm=True))
    for r in out:
        assert r["rc"] == 0, r.get("msg")
    return out
