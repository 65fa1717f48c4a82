"""Track driving and the telemetry handler with a per-car horizon on the device (mpc_drive_batch_device_horizon / _fused_horizon /
_host_horizon, mpc_telemetry_batch_device_horizon / _host_horizon; include/mpc_amd_drive.h): horizon = NULL against the _latency forms;
a mixed batch against its uniform parts run through the existing _latency form on handles created with N = horizon[i]; the one launch
against the stepwise form bit for bit at every B; every step against the handler's own entry point; the stepwise form against the CPU
build (tests/drive_twin) solve by solve; horizons and cars no caller should send; the host forms, the Python layer, the refusals
that need a live handle, and an N = 25 handle whose ordinary solve starts in fp32."""
import ctypes as C
import itertools

import numpy as np
import pytest

import drive_helpers as D
import drive_horizon_helpers as DH
import drive_latency_helpers as DL
from drive_helpers import fast_params as _params, to_device as _t
from helpers import TOL_STEER
from horizon_helpers import LOOP_HORIZONS
from model_helpers import draw_rows

pytestmark = pytest.mark.gpu

F, I = D.SENTINEL, D.ISENTINEL
_drive, _same = DH.device_drive, DH.same
ONE_LAUNCH, STEPWISE = {"fused_launches": 1, "stepwise_loops": 0}, {"fused_launches": 0, "stepwise_loops": 1}
GROUP_N = (3, 5, 7, 10)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return D.load_drive_twin()


@pytest.fixture(scope="module")
def cars200(pkg, golden_dir, waypoints):
    params = _params(pkg, golden_dir)
    return (pkg.scenarios.track_starts(200, params, waypoints, seed=6), pkg.scenarios.weight_sweep(200, params, seed=91),
            draw_rows(params, 200, seed=9), DL.draw_latency(200), DH.mixed_horizons(200))


@pytest.mark.parametrize("warm", [0, 1])
def test_horizon_null_is_the_latency_form(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """B = 65, the three drive forms and the two telemetry forms, the default wave limit and wave_max_batch = -1: bitwise, and the same
    mpc_drive_info."""
    import torch
    car, weights, model, lat = (np.ascontiguousarray(a[:, :65]) for a in cars200[:4])
    comp = np.ascontiguousarray(lat[0])
    for params in (_params(pkg, golden_dir), _params(pkg, golden_dir, wave_max_batch=-1)):
        for form in ("device", "fused", "host"):
            for m, l in ((None, None), (model, lat)):
                a = _drive(pkg, params, waypoints, car, 3, torch_dev, horizon=None, model=m, latency=l, form=form, warm=warm, weights=weights)
                b = _drive(pkg, params, waypoints, car, 3, torch_dev, model=m, latency=l, form=form, entry="latency", warm=warm, weights=weights)
                _same(a, b)
                assert a["info"] == b["info"], (form, m is not None)
        # the telemetry forms: the raw entry points with horizon = NULL against the _latency forms, cold and from a warm buffer
        lib = pkg.library()
        px, py = D.window_points(waypoints, D.twin_window(D.load_drive_twin(), waypoints, car[0], car[1]))
        B = 65
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            rows = mpc.warm_rows()
            res = {}
            for name in ("latency", "horizon"):
                hz = (None,) if name == "horizon" else ()
                d_car, d_comp, d_m = _t(car, torch_dev), _t(comp, torch_dev), _t(model, torch_dev)
                wbuf = torch.zeros((rows, B), dtype=torch.float64, device=torch_dev)
                st = torch.full((B,), I, dtype=torch.int32, device=torch_dev)
                cmds = []
                for rep in range(2 if warm else 1):
                    d_px, d_py = _t(px, torch_dev), _t(py, torch_dev)
                    cmd = torch.full((2, B), F, dtype=torch.float64, device=torch_dev)
                    rc = getattr(lib, "mpc_telemetry_batch_device_" + name)(
                        mpc._h, B, B, 6, d_car.data_ptr(), 0.01, d_comp.data_ptr(), d_px.data_ptr(), d_py.data_ptr(), d_m.data_ptr(), *hz,
                        wbuf.data_ptr() if rep else None, st.data_ptr() if rep else None, wbuf.data_ptr(), B, None, cmd.data_ptr(), None, st.data_ptr(),
                        C.c_void_p(torch.cuda.current_stream(torch_dev).cuda_stream))
                    assert rc == 0, lib.mpc_last_error()
                    torch.cuda.synchronize()
                    cmds.append(cmd.cpu().numpy())
                h_cmd = np.full((2, B), F); h_st = np.full(B, I, dtype=np.int32)
                p = lambda a: a.ctypes.data
                rc = getattr(lib, "mpc_telemetry_batch_host_" + name)(mpc._h, B, B, 6, p(car), 0.01, p(comp), p(px), p(py),
                                                                      p(model), *hz, None, None, None, 0, None, p(h_cmd), p(h_st))
                assert rc == 0, lib.mpc_last_error()
                res[name] = (cmds, st.cpu().numpy(), wbuf.cpu().numpy(), h_cmd, h_st)
            for x, y in zip(res["latency"][0] + list(res["latency"][1:]), res["horizon"][0] + list(res["horizon"][1:])):
                assert x.tobytes() == y.tobytes()
            assert np.array_equal(res["horizon"][0][0], res["horizon"][3])       # (host form = device form)


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("form", ["device", "fused"])
def test_a_mixed_batch_is_its_uniform_parts(pkg, golden_dir, waypoints, cars200, torch_dev, warm, form):
    """B = 200, horizon (3, 5, 7, 10)[i % 4] -- every wave holds all four --, 5 steps, weights: car i is bitwise car i of the existing
    _latency form on a handle created with N = horizon[i] and f64_f32_start = 0; the cars of the other groups differ.  The cold stepwise
    case again with model and latency columns."""
    car, weights, model, lat = cars200[:4]
    hz = DH.mixed_horizons(200, GROUP_N)
    cases = [(None, None)] + ([(model, lat)] if (form == "device" and not warm) else [])
    for m, l in cases:
        mixed = _drive(pkg, _params(pkg, golden_dir), waypoints, car, 5, torch_dev, horizon=hz, model=m, latency=l, form=form, warm=warm, weights=weights)
        assert mixed["info"] == (ONE_LAUNCH if form == "fused" else STEPWISE)
        for n in GROUP_N:
            ref = _drive(pkg, _params(pkg, golden_dir, N=n, f64_f32_start=0), waypoints, car, 5, torch_dev, model=m, latency=l, form=form, entry="latency",
                         warm=warm, weights=weights)
            _same(mixed, ref, cars=np.nonzero(hz == n)[0])
            others = np.nonzero(hz != n)[0]
            assert not np.array_equal(mixed["car"][:, others], ref["car"][:, others])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_fused_equals_stepwise_bitwise(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The one launch writes the stepwise horizon loop's bits: ld = B + 3, steps 1 and 5, hist NULL and not, the four pairings of model
    and weights over those four cases, with and without latency -- and mpc_drive_info shows one fused launch for every B, B = 1
    included, at the default wave limit as well."""
    car, weights, model, lat = (a[:, :B] for a in cars200[:4])
    hz = cars200[4][:B]
    lane_p, wave_p = _params(pkg, golden_dir, wave_max_batch=-1), _params(pkg, golden_dir)
    pairs = [(None, None), (model, weights), (model, None), (None, weights)]
    for latency in (None, lat):
        for (steps, hist), (m, w) in zip(itertools.product((1, 5), (True, False)), pairs):
            a = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, horizon=hz, model=m, latency=latency, warm=warm, weights=w, hist=hist)
            b = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, horizon=hz, model=m, latency=latency, warm=warm, weights=w, hist=hist, form="fused")
            _same(a, b)
            assert a["info"] == STEPWISE and b["info"] == ONE_LAUNCH, (steps, hist)
    c = _drive(pkg, wave_p, waypoints, car, 5, torch_dev, horizon=hz, model=None, latency=lat, warm=warm, weights=weights, hist=False, form="fused")
    _same(b, c)
    assert c["info"] == ONE_LAUNCH
    _same(a, _drive(pkg, wave_p, waypoints, car, 5, torch_dev, horizon=hz, model=None, latency=lat, warm=warm, weights=weights, hist=False))


@pytest.fixture(scope="module")
def loop96(pkg, golden_dir, waypoints, torch_dev):
    """B = 96 cars x 6 messages with the horizons LOOP_HORIZONS[i % 5], cold and warm, the default wave limit: computed once."""
    params = _params(pkg, golden_dir)
    car = pkg.scenarios.track_starts(96, params, waypoints, seed=4)
    hz = DH.mixed_horizons(96)
    return params, car, hz, {w: _drive(pkg, params, waypoints, car, 6, torch_dev, horizon=hz, warm=w) for w in (0, 1)}


@pytest.mark.parametrize("warm", [0, 1])
def test_every_step_is_the_handlers_own_answer(pkg, waypoints, loop96, torch_dev, warm):
    """mpc_telemetry_batch_device_horizon on hist's car and window of step t, with the horizons and (warm) the loop's records in place,
    returns bitwise hist's cmd, status and iterations."""
    import torch
    params, car, hz, res = loop96
    hist = res[warm]["hist"]
    B = car.shape[1]
    d_hz = _t(hz, torch_dev, np.int32)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        wbuf = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=torch_dev)
        status = torch.empty((B,), dtype=torch.int32, device=torch_dev)
        for t in range(hist.shape[0]):
            px, py = D.window_points(waypoints, hist[t, D.REC_K].astype(np.int64))
            kw = dict(warm=wbuf if t > 0 else None, warm_status=status if t > 0 else None, warm_out=wbuf, status_out=status) if warm else {}
            r = mpc.telemetry_torch(_t(hist[t, :6], torch_dev), _t(px, torch_dev), _t(py, torch_dev), horizon=d_hz, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(r["cmd"].cpu().numpy(), hist[t, D.REC_CMD:D.REC_CMD + 2]), t
            assert np.array_equal(r["status"].cpu().numpy(), hist[t, D.REC_STATUS].astype(np.int32)), t
            st = mpc.stats()       # (the telemetry entry points have no iterations array: the call's sum and maximum)
            assert (int(st.iter_sum), int(st.iter_max)) == (int(hist[t, D.REC_ITERS].sum()), int(hist[t, D.REC_ITERS].max())), t


@pytest.mark.parametrize("warm", [0, 1])
def test_stepwise_against_the_cpu_build(pkg, twin, waypoints, loop96, warm):
    """Windows and statuses equal at every step; the replies compared solve by solve -- the CPU build re-run on the device's recorded
    car and window with the car's horizon -- within the bounds of tests/test_drive_latency_gpu.py::test_stepwise_against_the_cpu_build;
    the cars after every plant step against the CPU build's plant, 4 x its substeps ulp."""
    params, car, hz, res = loop96
    dev = res[warm]
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    lat = DH.default_latency(params, opts, 96)
    tw = DH.twin_drive_horizon(twin, params, waypoints, car, hz, 6, opts, wopts)
    assert np.array_equal(dev["hist"][:, D.REC_K], tw["hist"][:, D.REC_K]) and np.array_equal(dev["hist"][:, D.REC_STATUS], tw["hist"][:, D.REC_STATUS])
    assert dev["info"] == STEPWISE
    mem = {"warm": None, "status": None}
    d_steer = d_thr = 0.0
    from run_model_helpers import uniform_model
    for t in range(6):
        h = dev["hist"][t]
        assert np.array_equal(D.twin_window(D.load_drive_twin(), waypoints, h[0], h[1]), h[D.REC_K].astype(np.int32))
        r = DH.twin_handler_horizon(twin, params, waypoints, h[:6], lat[DL.COMP], h[D.REC_K], hz, opts, wopts, warm=mem["warm"] if warm else None,
                                    warm_status=mem["status"] if warm else None, want_warm=bool(warm))
        mem["warm"], mem["status"] = r["warm"], r["status"]
        assert np.array_equal(r["status"], h[D.REC_STATUS].astype(np.int32)), t
        ok = r["status"] == 0
        d_steer = max(d_steer, (np.abs(r["cmd"][0] - h[D.REC_CMD]) * params.max_steering)[ok].max())
        d_thr = max(d_thr, np.abs(r["cmd"][1] - h[D.REC_CMD + 1])[ok].max())
        assert np.abs(r["cte_epsi"] - h[D.REC_CTE:D.REC_EPSI + 1])[:, ok].max() <= 1e-9
        nxt = dev["hist"][t + 1, :6] if t < 5 else dev["car"]
        ref = DL.twin_plant_latency(twin, params, h[:6], h[D.REC_CMD:D.REC_CMD + 2], uniform_model(params, 96), lat, opts)
        assert (np.abs(nxt - ref) <= 4 * (lat[DL.SUB_OLD] + lat[DL.SUB_NEW])[None, :] * np.spacing(np.maximum(1.0, np.abs(ref)))).all(), t
        assert np.array_equal(nxt[4], h[D.REC_CMD] * params.max_steering) and np.array_equal(nxt[5], h[D.REC_CMD + 1])
    print("device vs CPU build, warm %d: max |d steer| %.3g rad, |d throttle| %.3g; statuses %s" % (
        warm, d_steer, d_thr, np.bincount(dev["hist"][:, D.REC_STATUS].astype(np.int64).ravel())))
    assert d_steer <= TOL_STEER and d_thr <= D.TOL_THROTTLE
    D.check_summary(dev, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("fused", [False, True])
def test_containment(fused):
    """Inputs the entry points promise to survive: the four unusable horizons (2, 0, -1, N + 1), a NaN position, a car 1e6 m off the
    track (drive_horizon_helpers.containment_case).  The launch ends, every such car carries a status -- INFEASIBLE at every step, with
    finite rows, for the four horizons --, and every other car is bitwise what it is in a batch without them.  Both forms.  The drives
    run in a child process under a time limit of its own (the clean and the dirty batch, cold and warm: four launches or loops, nothing
    looped) whose exit status the parent checks."""
    res = D.run_in_child("drive_horizon_helpers.child_runs", fused)
    cols, bad = DH.BAD_HORIZONS, DH.BAD_HORIZONS + DH.BAD_CARS
    for warm in (0, 1):
        a, b = res[warm, "clean"], res[warm, "dirty"]
        assert b["info"]["fused_launches"] == (1 if fused else 0)
        assert (b["status"][bad] != 0).all() and (b["summary"][7, bad] >= 1).all()
        assert (b["hist"][:, D.REC_STATUS][:, cols] == DH.INFEASIBLE).all() and (b["summary"][7, cols] == 4).all()
        for k in ("car", "summary", "hist"):
            assert np.isfinite(b[k][..., cols]).all(), k
        good = np.setdiff1d(np.arange(a["status"].shape[0]), bad)
        _same(a, b, cars=good)


def test_host_form_and_python_layer(pkg, golden_dir, waypoints, cars200, torch_dev):
    """_host_horizon is bitwise the device form at B = 7; drive_torch(horizon=...) and drive_numpy(horizon=...) give the same results;
    telemetry_numpy(horizon=...) is telemetry_torch(horizon=...); shape and dtype errors raise ValueError."""
    import torch
    params = _params(pkg, golden_dir)
    car, weights, model, lat = (a[:, :7] for a in cars200[:4])
    hz = cars200[4][:7]
    tx, ty = D.track_of(waypoints)
    for warm in (0, 1):
        dev = _drive(pkg, params, waypoints, car, 3, torch_dev, horizon=hz, model=model, latency=lat, warm=warm, weights=weights)
        _same(dev, _drive(pkg, params, waypoints, car, 3, torch_dev, horizon=hz, model=model, latency=lat, warm=warm, weights=weights, form="host"))
        bare = _drive(pkg, params, waypoints, car, 3, torch_dev, horizon=hz, warm=warm)
        _same(bare, _drive(pkg, params, waypoints, car, 3, torch_dev, horizon=hz, warm=warm, form="host"))
        with pkg.BatchedMPC(params, 7, device=0) as mpc:
            o = mpc.drive_opts(warm_start=warm)
            for fused in (False, True):
                r = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, weights=_t(weights, torch_dev), opts=o, fused=fused,
                                    model=_t(model, torch_dev), latency=_t(lat, torch_dev), horizon=_t(hz, torch_dev, np.int32))
                torch.cuda.synchronize()
                for k in DH.KEYS:
                    assert np.array_equal(r[k].cpu().numpy(), dev[k]), (k, fused)
            _same(mpc.drive_numpy(car, tx, ty, 3, weights=weights, opts=o, model=model, latency=lat, horizon=hz), dev)
            _same(mpc.drive_numpy(car, tx, ty, 3, opts=o, horizon=hz), bare)
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, horizon=_t(hz[:6], torch_dev, np.int32))
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, horizon=_t(hz, torch_dev, np.int64))
            with pytest.raises(ValueError):
                mpc.drive_numpy(car, tx, ty, 3, horizon=hz[:6])
    px, py = D.window_points(waypoints, D.twin_window(D.load_drive_twin(), waypoints, car[0], car[1]))
    with pkg.BatchedMPC(params, 7, device=0) as mpc:
        a = mpc.telemetry_torch(_t(car, torch_dev), _t(px, torch_dev), _t(py, torch_dev), comp=_t(lat[0], torch_dev), model=_t(model, torch_dev),
                                horizon=_t(hz, torch_dev, np.int32))
        torch.cuda.synchronize()
        b = mpc.telemetry_numpy(car, px, py, comp=lat[0], model=model, horizon=hz)
        assert np.array_equal(a["cmd"].cpu().numpy(), b["cmd"]) and np.array_equal(a["status"].cpu().numpy(), b["status"]) and (b["status"] == 0).all()
        e = mpc.telemetry_numpy(car, px, py, comp=lat[0], model=model)
        assert not np.array_equal(b["cmd"], e["cmd"])                       # the horizon reaches the solve
        c = mpc.telemetry_numpy(car, px, py, horizon=hz)                    # ... and stands on its own
        g = mpc.telemetry_torch(_t(car, torch_dev), _t(px, torch_dev), _t(py, torch_dev), horizon=_t(hz, torch_dev, np.int32))
        torch.cuda.synchronize()
        assert np.array_equal(g["cmd"].cpu().numpy(), c["cmd"])
        with pytest.raises(ValueError):
            mpc.telemetry_torch(_t(car, torch_dev), _t(px, torch_dev), _t(py, torch_dev), horizon=_t(hz[:6], torch_dev, np.int32))
        with pytest.raises(ValueError):
            mpc.telemetry_numpy(car, px, py, horizon=hz[:6])


def test_refusals_on_a_live_handle(pkg, golden_dir, waypoints, torch_dev):
    """An F32 handle: MPC_ERR_INVALID with the model message; max_soc = 1 with a horizon: MPC_ERR_UNSUPPORTED with the message that names
    both; max_soc = 1 with horizon = NULL: served as before.  A refused call touches nothing."""
    import torch
    lib = pkg.library()
    tx, ty = D.track_of(waypoints)
    B = 8
    params = _params(pkg, golden_dir)
    car = _t(pkg.scenarios.track_starts(B, params, waypoints), torch_dev)
    hz = _t(DH.mixed_horizons(B), torch_dev, np.int32)
    d_tx, d_ty = _t(tx, torch_dev), _t(ty, torch_dev)
    px, py = D.window_points(waypoints, np.zeros(B, dtype=np.int64))
    d_px, d_py = _t(px, torch_dev), _t(py, torch_dev)
    summ = torch.full((8, B), F, dtype=torch.float64, device=torch_dev); st = torch.full((B,), I, dtype=torch.int32, device=torch_dev)
    cmd = torch.full((2, B), F, dtype=torch.float64, device=torch_dev)
    before, px_before = car.clone(), d_px.clone()
    NAMES = ("mpc_drive_batch_device_horizon", "mpc_drive_batch_device_fused_horizon")

    def drive(h, opts, name, horizon=hz):
        return getattr(lib, name)(h, B, B, 2, car.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(), len(tx), None, None,
                                  horizon.data_ptr() if horizon is not None else None, None, C.byref(opts), None, summ.data_ptr(), None, st.data_ptr(),
                                  None, None)

    def tel(h, horizon=hz):
        return lib.mpc_telemetry_batch_device_horizon(h, B, B, 6, car.data_ptr(), 0.0, None, d_px.data_ptr(), d_py.data_ptr(), None,
                                                      horizon.data_ptr() if horizon is not None else None, None, None, None, 0, None, cmd.data_ptr(),
                                                      None, st.data_ptr(), None)

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(car, before) and torch.equal(d_px, px_before) and bool((summ == F).all()) and bool((st == I).all()) and bool((cmd == F).all())
    good = pkg.drive_opts_default(params)
    with pkg.BatchedMPC(_params(pkg, golden_dir, precision=pkg.PRECISION_F32), B, device=0) as mpc:
        for name in NAMES:
            assert drive(mpc._h, good, name) == -1 and b"per-instance model values: fp64 handles only" in lib.mpc_last_error()
        assert tel(mpc._h) == -1 and b"per-instance model values: fp64 handles only" in lib.mpc_last_error()
        assert untouched() and mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
    with pkg.BatchedMPC(_params(pkg, golden_dir, max_soc=1), B, device=0) as mpc:
        for name in NAMES:
            assert drive(mpc._h, good, name) == -4 and b"per-instance horizon is not available with the second-order correction" in lib.mpc_last_error()
        assert tel(mpc._h) == -4 and b"per-instance horizon is not available with the second-order correction" in lib.mpc_last_error()
        assert untouched() and mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
        # horizon = NULL on the same handle: the _latency form's behaviour -- a warm call refused, a cold drive served by the stepwise loop
        assert tel(mpc._h, None) == -4 and b"warm start is not available with the second-order correction" in lib.mpc_last_error()
        assert drive(mpc._h, pkg.drive_opts_default(params, warm_start=1), NAMES[0], None) == -4 and b"second-order" in lib.mpc_last_error()
        assert untouched()
        assert drive(mpc._h, good, NAMES[1], None) == 0
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and mpc.drive_info() == STEPWISE


def test_a_handle_that_starts_in_fp32(pkg, golden_dir, waypoints, torch_dev):
    """An N = 25 handle with f64_f32_start at its default (the fp32 start for ordinary solves), B = 65, horizons from {3, 10, 17, 25},
    3 steps: bitwise the same call on a handle created with f64_f32_start = 0 -- the model rule -- stepwise and in one launch."""
    auto = _params(pkg, golden_dir, N=25)
    off = _params(pkg, golden_dir, N=25, f64_f32_start=0)
    car = pkg.scenarios.track_starts(65, auto, waypoints, seed=6)
    hz = DH.mixed_horizons(65, (3, 10, 17, 25))
    for warm in (0, 1):
        for form, info in (("device", STEPWISE), ("fused", ONE_LAUNCH)):
            a = _drive(pkg, auto, waypoints, car, 3, torch_dev, horizon=hz, form=form, warm=warm)
            b = _drive(pkg, off, waypoints, car, 3, torch_dev, horizon=hz, form=form, warm=warm)
            _same(a, b)
            assert a["info"] == b["info"] == info
