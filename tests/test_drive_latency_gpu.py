"""Track driving and the telemetry handler with per-car latency on the device (mpc_drive_batch_device_latency / _fused_latency /
_host_latency, mpc_telemetry_batch_device_latency / _host_latency; include/mpc_amd_drive.h): latency = NULL against the _model forms;
uniform columns against the call's scalars; a mixed batch against its uniform parts run through the existing _model form; the one
launch against the stepwise form bit for bit, across the wave limit and with ragged leading dimensions; every step against the
handler's own entry point; the stepwise form against the CPU build (tests/drive_twin) solve by solve; columns and cars no
caller should send; the host form, the Python layer and the refusals that need a live handle."""
import ctypes as C
import itertools

import numpy as np
import pytest

import drive_helpers as D
import drive_latency_helpers as DL
from drive_helpers import fast_params as _params, to_device as _t
from helpers import TOL_STEER
from model_helpers import draw_rows
from run_model_helpers import uniform_model

pytestmark = pytest.mark.gpu

F, I = D.SENTINEL, D.ISENTINEL
_drive, _same = DL.device_drive, DL.same
ONE_LAUNCH, STEPWISE = {"fused_launches": 1, "stepwise_loops": 0}, {"fused_launches": 0, "stepwise_loops": 1}


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
            draw_rows(params, 200, seed=9), DL.draw_latency(200))


@pytest.mark.parametrize("warm", [0, 1])
def test_latency_null_is_the_model_form(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """B = 65, all three forms, the wave kernels and the lane kernels, with and without model: bitwise, and the same dispatch."""
    car, weights, model = cars200[0][:, :65], cars200[1][:, :65], cars200[2][:, :65]
    for params in (_params(pkg, golden_dir), _params(pkg, golden_dir, wave_max_batch=-1)):
        for form in ("device", "fused", "host"):
            for m in (None, model):
                a = _drive(pkg, params, waypoints, car, 3, torch_dev, model=m, latency=None, form=form, warm=warm, weights=weights)
                b = _drive(pkg, params, waypoints, car, 3, torch_dev, model=m, form=form, entry="model", warm=warm, weights=weights)
                _same(a, b)
                assert a["info"] == b["info"], (form, m is not None)


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("latency_ms", [100, 0])
def test_uniform_columns_are_the_scalars(pkg, golden_dir, waypoints, cars200, torch_dev, warm, latency_ms):
    """A uniform column (lookahead + extra_latency, or 0 on a handle with latency_ms = 0; O.sub_old; O.sub_new) is bitwise the _model
    form: the stepwise loop on the wave kernels and the one launch."""
    car, model = cars200[0][:, :65], cars200[2][:, :65]
    over = dict(extra_latency=0.013, sub_old=7, sub_new=5)
    for wave, form, info in ((0, "device", STEPWISE), (-1, "fused", ONE_LAUNCH)):
        params = _params(pkg, golden_dir, wave_max_batch=wave, latency_ms=latency_ms)
        lat = DL.uniform_latency(65, DL.handle_comp(params, 0.013), 7, 5)
        assert lat[0, 0] == (0.0 if latency_ms == 0 else params.lookahead + 0.013)
        for m in (None, model):
            a = _drive(pkg, params, waypoints, car, 4, torch_dev, model=m, latency=lat, form=form, warm=warm, opts_over=over)
            b = _drive(pkg, params, waypoints, car, 4, torch_dev, model=m, form=form, entry="model", warm=warm, opts_over=over)
            _same(a, b)
            assert a["info"] == b["info"] == info


GROUPS = ((0.0, 5, 7), (0.05, 10, 2), (0.1, 0, 10), (0.18, 20, 4))      # (comp [s], sub_old, sub_new) of cars i % 4 == g


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("form,wave", [("device", 0), ("fused", -1)])
def test_a_mixed_batch_is_its_uniform_parts(pkg, golden_dir, waypoints, cars200, torch_dev, warm, form, wave):
    """B = 200 cars in 4 interleaved groups with 4 different columns, one of them comp = 0: car i of the mixed _latency call is bitwise
    car i of the existing _model form on a handle with lookahead = 0.0, latency_ms = 100 (0 for the comp = 0 group) and
    opts.extra_latency = comp, sub_old, sub_new of its group.  5 steps; the stepwise loop on the wave kernels and the one launch."""
    car, weights = cars200[0], cars200[1]
    g_of = np.arange(200) % 4
    lat = np.ascontiguousarray(np.array([[GROUPS[g][r] for g in g_of] for r in range(3)], dtype=np.float64))
    mixed = _drive(pkg, _params(pkg, golden_dir, wave_max_batch=wave), waypoints, car, 5, torch_dev, latency=lat, form=form, warm=warm, weights=weights)
    assert mixed["info"] == (ONE_LAUNCH if form == "fused" else STEPWISE)
    for g, (comp, so, sn) in enumerate(GROUPS):
        params = _params(pkg, golden_dir, wave_max_batch=wave, lookahead=0.0, latency_ms=100 if comp > 0 else 0)
        ref = _drive(pkg, params, waypoints, car, 5, torch_dev, form=form, entry="model", warm=warm, weights=weights,
                     opts_over=dict(extra_latency=comp, sub_old=so, sub_new=sn))
        _same(mixed, ref, cars=np.nonzero(g_of == g)[0])
        others = np.nonzero(g_of != g)[0]
        assert not np.array_equal(mixed["car"][:, others], ref["car"][:, others])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_fused_equals_stepwise_bitwise(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The one launch writes the stepwise latency loop's bits: ld = B + 3, steps 1 and 5, hist NULL and not, with and without model and
    weights (every pairing of the two over the four (steps, hist) cases), wave_max_batch = -1 so that every size reaches the lane kernel
    -- and mpc_drive_info says that the one launch ran.  The columns reach the drive: the results differ from the call's own scalars."""
    car, weights, model, lat = (a[:, :B] for a in cars200)
    lane_p = _params(pkg, golden_dir, wave_max_batch=-1)
    pairs = [(None, None), (model, weights), (model, None), (None, weights)]
    for (steps, hist), (m, w) in zip(itertools.product((1, 5), (True, False)), pairs):
        a = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, model=m, latency=lat, warm=warm, weights=w, hist=hist)
        b = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, model=m, latency=lat, warm=warm, weights=w, hist=hist, form="fused")
        _same(a, b)
        assert a["info"] == STEPWISE and b["info"] == ONE_LAUNCH, (steps, hist)
    u = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, latency=None, warm=warm, weights=weights, hist=False, form="fused")
    assert not np.array_equal(u["car"], b["car"])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_lane_kernels_and_wave_kernels_write_the_same_bits(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The stepwise latency loop with wave_max_batch = -1 (the lane kernel) against the default limit (the wave kernel): ld = B + 3,
    5 steps, with model and weights and without -- the same bits; hist = NULL changes nothing else."""
    car, weights, model, lat = (a[:, :B] for a in cars200)
    lane_p, wave_p = _params(pkg, golden_dir, wave_max_batch=-1), _params(pkg, golden_dir)
    for m, w in ((None, None), (model, weights)):
        lane = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, model=m, latency=lat, warm=warm, weights=w)
        _same(lane, _drive(pkg, wave_p, waypoints, car, 5, torch_dev, model=m, latency=lat, warm=warm, weights=w))
        _same(lane, _drive(pkg, lane_p, waypoints, car, 5, torch_dev, model=m, latency=lat, warm=warm, weights=w, hist=False))
        assert lane["info"] == STEPWISE


@pytest.fixture(scope="module")
def loop96(pkg, golden_dir, waypoints, torch_dev):
    """B = 96 cars x 6 messages with the columns draw_latency(96, seed 23), cold and warm, the default wave limit: computed once."""
    params = _params(pkg, golden_dir)
    car = pkg.scenarios.track_starts(96, params, waypoints, seed=4)
    lat = DL.draw_latency(96, seed=23)
    return params, car, lat, {w: _drive(pkg, params, waypoints, car, 6, torch_dev, latency=lat, warm=w) for w in (0, 1)}


@pytest.mark.parametrize("warm", [0, 1])
def test_every_step_is_the_handlers_own_answer(pkg, waypoints, loop96, torch_dev, warm):
    """mpc_telemetry_batch_device_latency on hist's car and window of step t, with comp and (warm) the loop's records, returns bitwise
    hist's cmd, status and iterations -- under a handle whose own latency settings and extra_latency say something else."""
    import torch
    params, car, lat, res = loop96
    hist = res[warm]["hist"]
    B = car.shape[1]
    comp = _t(lat[DL.COMP], torch_dev)
    other = params.copy(); other.lookahead = 0.3
    with pkg.BatchedMPC(other, B, device=0) as mpc:
        wbuf = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=torch_dev)
        status = torch.empty((B,), dtype=torch.int32, device=torch_dev)
        for t in range(hist.shape[0]):
            px, py = D.window_points(waypoints, hist[t, D.REC_K].astype(np.int64))
            kw = dict(warm=wbuf if t > 0 else None, warm_status=status if t > 0 else None, warm_out=wbuf, status_out=status) if warm else {}
            r = mpc.telemetry_torch(_t(hist[t, :6], torch_dev), _t(px, torch_dev), _t(py, torch_dev), extra_latency=0.07, comp=comp, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(r["cmd"].cpu().numpy(), hist[t, D.REC_CMD:D.REC_CMD + 2]), t
            assert np.array_equal(r["status"].cpu().numpy(), hist[t, D.REC_STATUS].astype(np.int32)), t
            st = mpc.stats()       # (the telemetry entry points have no iterations array: the call's sum and maximum)
            assert (int(st.iter_sum), int(st.iter_max)) == (int(hist[t, D.REC_ITERS].sum()), int(hist[t, D.REC_ITERS].max())), t


@pytest.mark.parametrize("warm", [0, 1])
def test_stepwise_against_the_cpu_build(pkg, twin, waypoints, loop96, warm):
    """Windows and statuses equal at every step; the replies compared solve by solve -- the CPU build re-run on the device's recorded
    car and window with the car's comp -- within the bounds of tests/test_drive_gpu.py::test_stepwise_against_the_cpu_build; the cars
    after every plant step against the CPU build's plant with the car's own counts, 4 x its substeps ulp."""
    params, car, lat, res = loop96
    dev = res[warm]
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    model = uniform_model(params, 96)
    tw = DL.twin_drive_latency(twin, params, waypoints, car, model, lat, 6, opts, wopts)
    assert np.array_equal(dev["hist"][:, D.REC_K], tw["hist"][:, D.REC_K]) and np.array_equal(dev["hist"][:, D.REC_STATUS], tw["hist"][:, D.REC_STATUS])
    assert dev["info"] == STEPWISE
    mem = {"warm": None, "status": None}
    d_steer = d_thr = 0.0
    for t in range(6):
        h = dev["hist"][t]
        assert np.array_equal(D.twin_window(D.load_drive_twin(), waypoints, h[0], h[1]), h[D.REC_K].astype(np.int32))
        r = DL.twin_handler_latency(twin, params, waypoints, h[:6], lat[DL.COMP], h[D.REC_K], model, opts, wopts, warm=mem["warm"] if warm else None,
                                    warm_status=mem["status"] if warm else None, want_warm=bool(warm))
        mem["warm"], mem["status"] = r["warm"], r["status"]
        assert np.array_equal(r["status"], h[D.REC_STATUS].astype(np.int32)), t
        ok = r["status"] == 0
        d_steer = max(d_steer, (np.abs(r["cmd"][0] - h[D.REC_CMD]) * params.max_steering)[ok].max())
        d_thr = max(d_thr, np.abs(r["cmd"][1] - h[D.REC_CMD + 1])[ok].max())
        assert np.abs(r["cte_epsi"] - h[D.REC_CTE:D.REC_EPSI + 1])[:, ok].max() <= 1e-9
        nxt = dev["hist"][t + 1, :6] if t < 5 else dev["car"]
        ref = DL.twin_plant_latency(twin, params, h[:6], h[D.REC_CMD:D.REC_CMD + 2], model, lat, opts)
        assert (np.abs(nxt - ref) <= 4 * (lat[DL.SUB_OLD] + lat[DL.SUB_NEW])[None, :] * np.spacing(np.maximum(1.0, np.abs(ref)))).all(), t
        assert np.array_equal(nxt[4], h[D.REC_CMD] * params.max_steering) and np.array_equal(nxt[5], h[D.REC_CMD + 1])
    print("device vs CPU build, warm %d: max |d steer| %.3g rad, |d throttle| %.3g; statuses %s" % (
        warm, d_steer, d_thr, np.bincount(dev["hist"][:, D.REC_STATUS].astype(np.int64).ravel())))
    assert d_steer <= TOL_STEER and d_thr <= D.TOL_THROTTLE
    D.check_summary(dev, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("wave_max_batch,fused", [(0, False), (-1, False), (-1, True)])
def test_containment(pkg, golden_dir, waypoints, wave_max_batch, fused):
    """Inputs the entry points promise to survive: the four unusable columns (NaN, comp = -1, sub_old = 2.5, sub_old + sub_new = 1001), a
    NaN position, a car 1e6 m off the track (drive_latency_helpers.containment_case).  The launch ends, every such car carries a
    status -- at every step, with finite rows, for the four columns --, and every other car is bitwise what it is in a batch without
    them.  Both forms.  The drives run in a child process under a time limit of its own (the clean and the dirty batch, cold and
    warm: four launches or loops, nothing looped), so that "a launch that ends" is something this test can say."""
    res = D.run_in_child("drive_latency_helpers.child_runs", fused, wave_max_batch)
    cols, bad = DL.BAD_COLUMNS, DL.BAD_COLUMNS + DL.BAD_CARS
    for warm in (0, 1):
        a, b = res[warm, "clean"], res[warm, "dirty"]
        assert b["info"]["fused_launches"] == (1 if fused else 0)
        assert (b["status"][bad] != 0).all() and (b["summary"][7, bad] >= 1).all()
        assert (b["hist"][:, D.REC_STATUS][:, cols] != 0).all() and (b["summary"][7, cols] == 4).all()
        for k in ("car", "summary", "hist"):
            assert np.isfinite(b[k][..., cols]).all(), k
        good = np.setdiff1d(np.arange(a["status"].shape[0]), bad)
        _same(a, b, cars=good)


def test_host_form_and_python_layer(pkg, golden_dir, waypoints, cars200, torch_dev):
    """_host_latency is bitwise the device form at B = 7; drive_torch(latency=...) and drive_numpy(latency=...) give the same results;
    telemetry_numpy(comp=...) is telemetry_torch(comp=...); shape and dtype errors raise ValueError."""
    import torch
    params = _params(pkg, golden_dir)
    car, weights, model, lat = (a[:, :7] for a in cars200)
    tx, ty = D.track_of(waypoints)
    for warm in (0, 1):
        dev = _drive(pkg, params, waypoints, car, 3, torch_dev, model=model, latency=lat, warm=warm, weights=weights)
        _same(dev, _drive(pkg, params, waypoints, car, 3, torch_dev, model=model, latency=lat, warm=warm, weights=weights, form="host"))
        nomodel = _drive(pkg, params, waypoints, car, 3, torch_dev, latency=lat, warm=warm)
        with pkg.BatchedMPC(params, 7, device=0) as mpc:
            o = mpc.drive_opts(warm_start=warm)
            for fused in (False, True):
                r = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, weights=_t(weights, torch_dev), opts=o, fused=fused,
                                    model=_t(model, torch_dev), latency=_t(lat, torch_dev))
                torch.cuda.synchronize()
                for k in DL.KEYS:
                    assert np.array_equal(r[k].cpu().numpy(), dev[k]), (k, fused)
            n = mpc.drive_numpy(car, tx, ty, 3, weights=weights, opts=o, model=model, latency=lat)
            _same(n, dev)
            _same(mpc.drive_numpy(car, tx, ty, 3, opts=o, latency=lat), nomodel)
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, latency=_t(lat[:, :6], torch_dev))
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, latency=_t(lat, torch_dev).float())
            with pytest.raises(ValueError):
                mpc.drive_numpy(car, tx, ty, 3, latency=lat[:2])
    px, py = D.window_points(waypoints, D.twin_window(D.load_drive_twin(), waypoints, car[0], car[1]))
    with pkg.BatchedMPC(params, 7, device=0) as mpc:
        a = mpc.telemetry_torch(_t(car, torch_dev), _t(px, torch_dev), _t(py, torch_dev), comp=_t(lat[0], torch_dev), model=_t(model, torch_dev))
        torch.cuda.synchronize()
        b = mpc.telemetry_numpy(car, px, py, comp=lat[0], model=model)
        assert np.array_equal(a["cmd"].cpu().numpy(), b["cmd"]) and np.array_equal(a["status"].cpu().numpy(), b["status"]) and (b["status"] == 0).all()
        # comp = None through the _latency form is the handle's own rule: the plain telemetry call
        c = mpc.telemetry_torch(_t(car, torch_dev), _t(px, torch_dev), _t(py, torch_dev), extra_latency=0.01)
        torch.cuda.synchronize()
        e = mpc.telemetry_numpy(car, px, py, extra_latency=0.01)
        assert np.array_equal(c["cmd"].cpu().numpy(), e["cmd"]) and not np.array_equal(b["cmd"], e["cmd"])
        with pytest.raises(ValueError):
            mpc.telemetry_torch(_t(car, torch_dev), _t(px, torch_dev), _t(py, torch_dev), comp=_t(lat[0, :6], torch_dev))
        with pytest.raises(ValueError):
            mpc.telemetry_torch(_t(car, torch_dev), _t(px, torch_dev), _t(py, torch_dev), comp=_t(lat[0], torch_dev).float())
        with pytest.raises(ValueError):
            mpc.telemetry_numpy(car, px, py, comp=lat[:2])


def test_refusals_on_a_live_handle(pkg, golden_dir, waypoints, torch_dev):
    """An F32 handle: MPC_ERR_INVALID; warm_start (the telemetry form: always) with max_soc > 0: MPC_ERR_UNSUPPORTED; ld < B:
    MPC_ERR_INVALID.  A refused call touches nothing."""
    import torch
    lib = pkg.library()
    tx, ty = D.track_of(waypoints)
    B = 8
    params = _params(pkg, golden_dir)
    car = _t(pkg.scenarios.track_starts(B, params, waypoints), torch_dev)
    lat = _t(DL.draw_latency(B), torch_dev)
    d_tx, d_ty = _t(tx, torch_dev), _t(ty, torch_dev)
    px, py = D.window_points(waypoints, np.zeros(B, dtype=np.int64))
    d_px, d_py = _t(px, torch_dev), _t(py, torch_dev)
    summ = torch.full((8, B), F, dtype=torch.float64, device=torch_dev); st = torch.full((B,), I, dtype=torch.int32, device=torch_dev)
    cmd = torch.full((2, B), F, dtype=torch.float64, device=torch_dev)
    before, px_before = car.clone(), d_px.clone()

    def drive(h, opts, name, ld=B):
        return getattr(lib, name)(h, B, ld, 2, car.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(), len(tx), None, None, lat.data_ptr(), C.byref(opts), None,
                                  summ.data_ptr(), None, st.data_ptr(), None, None)

    def tel(h, ld=B):
        return lib.mpc_telemetry_batch_device_latency(h, B, ld, 6, car.data_ptr(), 0.0, lat.data_ptr(), d_px.data_ptr(), d_py.data_ptr(), None, None, None,
                                                      None, 0, None, cmd.data_ptr(), None, st.data_ptr(), None)

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(car, before) and torch.equal(d_px, px_before) and bool((summ == F).all()) and bool((st == I).all()) and bool((cmd == F).all())
    good = pkg.drive_opts_default(params)
    with pkg.BatchedMPC(_params(pkg, golden_dir, precision=pkg.PRECISION_F32), B, device=0) as mpc:
        for name in ("mpc_drive_batch_device_latency", "mpc_drive_batch_device_fused_latency"):
            assert drive(mpc._h, good, name) == -1 and b"fp64 handles only" in lib.mpc_last_error()
        assert tel(mpc._h) == -1 and b"per-instance latency: fp64 handles only" in lib.mpc_last_error()
        assert untouched() and mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        for name in ("mpc_drive_batch_device_latency", "mpc_drive_batch_device_fused_latency"):
            assert drive(mpc._h, good, name, ld=B - 1) == -1 and b"ld" in lib.mpc_last_error()
            bad = pkg.drive_opts_default(params, sub_old=-1)                 # the call's own scalars are still validated
            assert drive(mpc._h, bad, name) == -1 and b"substep" in lib.mpc_last_error()
        assert tel(mpc._h, ld=B - 1) == -1 and b"ld" in lib.mpc_last_error()
        assert untouched() and mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
    with pkg.BatchedMPC(_params(pkg, golden_dir, max_soc=4), B, device=0) as mpc:
        for name in ("mpc_drive_batch_device_latency", "mpc_drive_batch_device_fused_latency"):
            assert drive(mpc._h, pkg.drive_opts_default(params, warm_start=1), name) == -4 and b"second-order" in lib.mpc_last_error()
        assert tel(mpc._h) == -4 and b"second-order" in lib.mpc_last_error()
        assert untouched()
        assert drive(mpc._h, good, "mpc_drive_batch_device_latency") == 0          # cold with SOC: served, by the stepwise loop
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and mpc.drive_info() == STEPWISE
