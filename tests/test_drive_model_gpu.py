"""Track driving with per-car model values on the device (mpc_drive_batch_device_model / _fused_model / _host_model,
include/mpc_amd_drive.h): the stepwise form against the CPU build of the same functions (tests/drive_twin) solve by solve and
against the telemetry _model entry points bit for bit; model = NULL against the forms without _model; the one launch (the DRIVE x
MODEL builds of the lane kernel) against the stepwise form bit for bit, across the wave limit and with ragged leading dimensions;
columns and cars no caller should send; the host form, the Python layer and the refusals that need a live handle."""
import ctypes as C

import numpy as np
import pytest

import drive_helpers as D
import drive_model_helpers as DM
from helpers import TOL_STEER
from model_helpers import INFEASIBLE, draw_rows
from run_model_helpers import uniform_model

pytestmark = pytest.mark.gpu

F, I = D.SENTINEL, D.ISENTINEL
_t, _params, _drive = DM.to_device, DM.fast_params, DM.device_drive
KEYS = ("car", "summary", "hist", "status", "iters")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return D.load_drive_twin()


def _same(a, b, what=""):
    for k in KEYS:
        if a[k] is not None and b[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


ONE_LAUNCH, STEPWISE = {"fused_launches": 1, "stepwise_loops": 0}, {"fused_launches": 0, "stepwise_loops": 1}


@pytest.fixture(scope="module")
def loop96(pkg, golden_dir, waypoints, torch_dev):
    """B = 96 cars x 6 messages with the columns draw_rows(seed 9), cold and warm, the default wave limit: computed once, shared."""
    params = _params(pkg, golden_dir)
    car = pkg.scenarios.track_starts(96, params, waypoints, seed=4)
    model = draw_rows(params, 96, seed=9)
    return params, car, model, {w: _drive(pkg, params, waypoints, car, model, 6, torch_dev, warm=w) for w in (0, 1)}


@pytest.mark.parametrize("warm", [0, 1])
def test_stepwise_against_the_cpu_build(pkg, twin, waypoints, loop96, warm):
    """Windows and statuses equal at every step; the replies compared solve by solve -- the CPU build re-run on the device's recorded
    car and window -- within the bounds of tests/test_drive_gpu.py::test_stepwise_against_the_cpu_build (the steer in radians of the
    car's own max_steering); the cars after every plant step bitwise follow from the records (row 4: cmd_steer x max_steering_i)."""
    params, car, model, res = loop96
    dev = res[warm]
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    tw = DM.twin_drive_model(twin, params, waypoints, car, model, 6, opts, wopts)
    assert np.array_equal(dev["hist"][:, D.REC_K], tw["hist"][:, D.REC_K]) and np.array_equal(dev["hist"][:, D.REC_STATUS], tw["hist"][:, D.REC_STATUS])
    assert dev["info"] == STEPWISE
    mem = {"warm": None, "status": None}
    d_steer = d_thr = 0.0
    for t in range(6):
        h = dev["hist"][t]
        assert np.array_equal(D.twin_window(D.load_drive_twin(), waypoints, h[0], h[1]), h[D.REC_K].astype(np.int32))
        r = DM.twin_handler_model(twin, params, waypoints, h[:6], h[D.REC_K], model, opts, wopts, warm=mem["warm"] if warm else None,
                                  warm_status=mem["status"] if warm else None, want_warm=bool(warm))
        mem["warm"], mem["status"] = r["warm"], r["status"]
        assert np.array_equal(r["status"], h[D.REC_STATUS].astype(np.int32)), t
        ok = r["status"] == 0
        d_steer = max(d_steer, (np.abs(r["cmd"][0] - h[D.REC_CMD]) * model[2])[ok].max())
        d_thr = max(d_thr, np.abs(r["cmd"][1] - h[D.REC_CMD + 1])[ok].max())
        assert np.abs(r["cte_epsi"] - h[D.REC_CTE:D.REC_EPSI + 1])[:, ok].max() <= 1e-9
        # the plant: the device's next car against the CPU build's plant on the device's own car and reply, 4 x substeps ulp
        nxt = dev["hist"][t + 1, :6] if t < 5 else dev["car"]
        ref = DM.twin_plant_model(twin, params, h[:6], h[D.REC_CMD:D.REC_CMD + 2], model, opts.sub_old, opts.sub_new, opts.h)
        assert (np.abs(nxt - ref) <= 4 * (opts.sub_old + opts.sub_new) * np.spacing(np.maximum(1.0, np.abs(ref)))).all(), t
        assert np.array_equal(nxt[4], h[D.REC_CMD] * model[2]) and np.array_equal(nxt[5], h[D.REC_CMD + 1])
    print("device vs CPU build, warm %d: max |d steer| %.3g rad, |d throttle| %.3g; statuses %s" % (
        warm, d_steer, d_thr, np.bincount(dev["hist"][:, D.REC_STATUS].astype(np.int64).ravel())))
    assert d_steer <= TOL_STEER and d_thr <= D.TOL_THROTTLE
    D.check_summary(dev, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("warm", [0, 1])
def test_every_step_is_the_handlers_own_answer(pkg, waypoints, loop96, torch_dev, warm):
    """mpc_telemetry_batch_device_model (warm: _warm_model with the loop's records) on hist's car and window of step t returns bitwise
    hist's cmd, status and iterations."""
    import torch
    params, car, model, res = loop96
    hist = res[warm]["hist"]
    B = car.shape[1]
    d_model = _t(model, torch_dev)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        wbuf = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=torch_dev)
        status = torch.empty((B,), dtype=torch.int32, device=torch_dev)
        for t in range(hist.shape[0]):
            px, py = D.window_points(waypoints, hist[t, D.REC_K].astype(np.int64))
            kw = dict(warm=wbuf if t > 0 else None, warm_status=status if t > 0 else None, warm_out=wbuf, status_out=status) if warm else {}
            r = mpc.telemetry_torch(_t(hist[t, :6], torch_dev), _t(px, torch_dev), _t(py, torch_dev), model=d_model, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(r["cmd"].cpu().numpy(), hist[t, D.REC_CMD:D.REC_CMD + 2]), t
            assert np.array_equal(r["status"].cpu().numpy(), hist[t, D.REC_STATUS].astype(np.int32)), t
            st = mpc.stats()       # (the telemetry entry points have no iterations array: the call's sum and maximum)
            assert (int(st.iter_sum), int(st.iter_max)) == (int(hist[t, D.REC_ITERS].sum()), int(hist[t, D.REC_ITERS].max())), t


@pytest.fixture(scope="module")
def cars200(pkg, golden_dir, waypoints):
    params = _params(pkg, golden_dir)
    return (pkg.scenarios.track_starts(200, params, waypoints, seed=6), pkg.scenarios.weight_sweep(200, params, seed=91),
            draw_rows(params, 200, seed=9))


@pytest.mark.parametrize("warm", [0, 1])
def test_model_null_is_the_form_without_model(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """B = 65, all three forms, the wave kernels and the lane kernels: bitwise, and the same dispatch."""
    car, weights = cars200[0][:, :65], cars200[1][:, :65]
    for params in (_params(pkg, golden_dir), _params(pkg, golden_dir, wave_max_batch=-1)):
        for kw in (dict(), dict(fused=True), dict(host=True)):
            a = _drive(pkg, params, waypoints, car, None, 3, torch_dev, warm=warm, weights=weights, **kw)
            b = _drive(pkg, params, waypoints, car, None, 3, torch_dev, warm=warm, weights=weights, plain=True, **kw)
            _same(a, b, "model = NULL %s" % kw)
            assert a["info"] == b["info"]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_fused_equals_stepwise_bitwise(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The one launch writes the stepwise model loop's bits: ld = B + 3, steps 1 and 5, hist NULL and not, with and without
    per-instance weights, wave_max_batch = -1 so that every size reaches the lane kernel -- and mpc_drive_info says that the one launch
    ran.  The columns reach the drive: the results differ from those of the handle's own values."""
    car, weights, model = cars200[0][:, :B], cars200[1][:, :B], cars200[2][:, :B]
    lane_p = _params(pkg, golden_dir, wave_max_batch=-1)
    for steps in (1, 5):
        for hist in (True, False):
            for w in (None, weights):
                a = _drive(pkg, lane_p, waypoints, car, model, steps, torch_dev, warm=warm, weights=w, hist=hist)
                b = _drive(pkg, lane_p, waypoints, car, model, steps, torch_dev, warm=warm, weights=w, hist=hist, fused=True)
                _same(a, b, "fused / stepwise, steps %d hist %s weights %s" % (steps, hist, w is not None))
                assert a["info"] == STEPWISE and b["info"] == ONE_LAUNCH
    u = _drive(pkg, lane_p, waypoints, car, uniform_model(lane_p, B), 5, torch_dev, warm=warm, fused=True)
    assert not np.array_equal(u["car"], b["car"])
    _same(u, _drive(pkg, lane_p, waypoints, car, None, 5, torch_dev, warm=warm, fused=True, plain=True), "uniform columns / no model")


@pytest.mark.parametrize("warm", [0, 1])
def test_fused_call_below_the_wave_limit_runs_the_stepwise_loop(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """With the default wave limit and B = 65 the fused model call runs the stepwise loop itself, says so, and the bits are equal --
    to the stepwise call and to the one launch of a handle without the wave path."""
    car, model = cars200[0][:, :65], cars200[2][:, :65]
    a = _drive(pkg, _params(pkg, golden_dir), waypoints, car, model, 5, torch_dev, warm=warm)
    b = _drive(pkg, _params(pkg, golden_dir), waypoints, car, model, 5, torch_dev, warm=warm, fused=True)
    c = _drive(pkg, _params(pkg, golden_dir, wave_max_batch=-1), waypoints, car, model, 5, torch_dev, warm=warm, fused=True)
    assert b["info"] == STEPWISE and c["info"] == ONE_LAUNCH
    _same(a, b, "fused call, wave path"); _same(a, c, "one launch against the wave kernels")


@pytest.mark.parametrize("warm", [0, 1])
def test_one_launch_on_a_handle_that_starts_in_fp32(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """N = 15 with default parameters (f64_f32_start = AUTO: the ordinary solve is the two-launch fp32-start solve, and the fused call
    without model runs the stepwise loop there): the model call runs the one launch, bitwise a handle with f64_f32_start = 0 and
    bitwise its own stepwise loop."""
    car, model = cars200[0][:, :65], cars200[2][:, :65]
    p = _params(pkg, golden_dir, N=15, wave_max_batch=-1)
    assert p.f64_f32_start == 2
    a = _drive(pkg, p, waypoints, car, model, 3, torch_dev, warm=warm, fused=True)
    b = _drive(pkg, _params(pkg, golden_dir, N=15, wave_max_batch=-1, f64_f32_start=0), waypoints, car, model, 3, torch_dev, warm=warm, fused=True)
    assert a["info"] == ONE_LAUNCH and b["info"] == ONE_LAUNCH
    _same(a, b, "fp32-start handle / f64_f32_start = 0")
    _same(a, _drive(pkg, p, waypoints, car, model, 3, torch_dev, warm=warm), "one launch / stepwise on the fp32-start handle")
    if not warm:
        assert _drive(pkg, p, waypoints, car, None, 3, torch_dev, fused=True, plain=True)["info"] == STEPWISE


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_lane_kernels_and_wave_kernels_write_the_same_bits(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The stepwise model loop with wave_max_batch = -1 (the lane kernel's MODEL build) against the default limit (the wave kernel's
    MODEL build): ld = B + 3, 5 steps, with and without weights -- the same bits; hist = NULL changes nothing else."""
    car, weights, model = cars200[0][:, :B], cars200[1][:, :B], cars200[2][:, :B]
    lane_p, wave_p = _params(pkg, golden_dir, wave_max_batch=-1), _params(pkg, golden_dir)
    for w in (None, weights):
        lane = _drive(pkg, lane_p, waypoints, car, model, 5, torch_dev, warm=warm, weights=w)
        _same(lane, _drive(pkg, wave_p, waypoints, car, model, 5, torch_dev, warm=warm, weights=w), "lane / wave")
        _same(lane, _drive(pkg, lane_p, waypoints, car, model, 5, torch_dev, warm=warm, weights=w, hist=False), "hist = NULL")
        assert lane["info"] == STEPWISE


@pytest.mark.parametrize("wave_max_batch,fused", [(0, False), (-1, False), (-1, True)])
def test_containment(pkg, golden_dir, waypoints, wave_max_batch, fused):
    """Inputs the entry points promise to survive: an unusable column (NaN; dt = 0), a car above its own relaxed speed limit, a NaN
    position, a car 1e6 m off the track (drive_model_helpers.containment_case).  The launch ends, every such car carries a status --
    INFEASIBLE at every step with finite rows for the first three --, and every other car is bitwise what it is in a batch without
    them.  Both forms.  The drives run in a child process under a time limit of its own (the clean and the dirty batch, cold and
    warm: four launches or loops), so that "a launch that ends" is something this test can say."""
    res = D.run_in_child("drive_model_helpers.child_runs", fused, wave_max_batch)
    _, _, _, _, infeasible, bad = DM.containment_case(pkg, _params(pkg, golden_dir, wave_max_batch=wave_max_batch), waypoints)
    for warm in (0, 1):
        a, b = res[warm, "clean"], res[warm, "dirty"]
        assert b["info"]["fused_launches"] == (1 if fused else 0)
        assert (b["status"][bad] != 0).all() and (b["summary"][7, bad] >= 1).all()
        assert (b["hist"][:, D.REC_STATUS][:, infeasible] == INFEASIBLE).all()
        for k in ("car", "summary", "hist"):
            assert np.isfinite(b[k][..., infeasible]).all(), k
        good = np.setdiff1d(np.arange(a["status"].shape[0]), bad)
        for k in KEYS:
            assert np.array_equal(a[k][..., good], b[k][..., good]), k
        assert (a["status"] == 0).all()


def test_host_form_and_python_layer(pkg, golden_dir, waypoints, cars200, torch_dev):
    """_host_model is bitwise the device form at B = 7; drive_torch(model=...) and drive_numpy(model=...) give the same results."""
    import torch
    params = _params(pkg, golden_dir)
    car, weights, model = cars200[0][:, :7], cars200[1][:, :7], cars200[2][:, :7]
    tx, ty = D.track_of(waypoints)
    for warm in (0, 1):
        dev = _drive(pkg, params, waypoints, car, model, 3, torch_dev, warm=warm, weights=weights)
        _same(dev, _drive(pkg, params, waypoints, car, model, 3, torch_dev, warm=warm, weights=weights, host=True), "host form")
        with pkg.BatchedMPC(params, 7, device=0) as mpc:
            o = mpc.drive_opts(warm_start=warm)
            for fused in (False, True):
                r = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, weights=_t(weights, torch_dev), opts=o, fused=fused,
                                    model=_t(model, torch_dev))
                torch.cuda.synchronize()
                for k in KEYS:
                    assert np.array_equal(r[k].cpu().numpy(), dev[k]), (k, fused)
            n = mpc.drive_numpy(car, tx, ty, 3, weights=weights, opts=o, model=model)
            for k in KEYS:
                assert np.array_equal(n[k], dev[k]), k
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, model=_t(model[:, :6], torch_dev))
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, model=_t(model, torch_dev).float())
            with pytest.raises(ValueError):
                mpc.drive_numpy(car, tx, ty, 3, model=model[:5])


def test_refusals_on_a_live_handle(pkg, golden_dir, waypoints, torch_dev):
    """An F32 handle: MPC_ERR_INVALID with the model message; warm_start with max_soc > 0: MPC_ERR_UNSUPPORTED; ld < B: the refusal of
    the form without _model.  A refused call touches nothing."""
    import torch
    lib = pkg.library()
    tx, ty = D.track_of(waypoints)
    B = 8
    params = _params(pkg, golden_dir)
    car = _t(pkg.scenarios.track_starts(B, params, waypoints), torch_dev)
    model = _t(uniform_model(params, B), torch_dev)
    d_tx, d_ty = _t(tx, torch_dev), _t(ty, torch_dev)
    summ = torch.full((8, B), F, dtype=torch.float64, device=torch_dev); st = torch.full((B,), I, dtype=torch.int32, device=torch_dev)
    before = car.clone()

    def call(h, opts, name="mpc_drive_batch_device_model", ld=B):
        return getattr(lib, name)(h, B, ld, 2, car.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(), len(tx), None, model.data_ptr(), C.byref(opts), None,
                                  summ.data_ptr(), None, st.data_ptr(), None, None)
    good = pkg.drive_opts_default(params)
    for name in ("mpc_drive_batch_device_model", "mpc_drive_batch_device_fused_model"):
        with pkg.BatchedMPC(_params(pkg, golden_dir, precision=pkg.PRECISION_F32), B, device=0) as mpc:
            assert call(mpc._h, good, name) == -1 and b"per-instance model values: fp64 handles only" in lib.mpc_last_error()
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            assert call(mpc._h, good, name, ld=B - 1) == -1 and b"ld" in lib.mpc_last_error()
            assert mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
        with pkg.BatchedMPC(_params(pkg, golden_dir, max_soc=4), B, device=0) as mpc:
            assert call(mpc._h, pkg.drive_opts_default(params, warm_start=1), name) == -4 and b"second-order" in lib.mpc_last_error()
            torch.cuda.synchronize()
            assert torch.equal(car, before) and (summ == F).all() and (st == I).all()      # a refused call touches nothing
            assert call(mpc._h, good, name) == 0                                           # cold with SOC: served, by the stepwise loop
            torch.cuda.synchronize()
            assert (st.cpu().numpy() == 0).all() and mpc.drive_info() == STEPWISE
            car.copy_(before); summ.fill_(F); st.fill_(I)
