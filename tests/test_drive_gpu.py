"""Track driving on the device (mpc_drive_batch_device / _fused / _host, include/mpc_amd_drive.h): the stepwise form -- the two drive
kernels around the handler's three launches -- against the CPU build of the same functions (tests/drive_twin) solve by solve and
against the telemetry entry points themselves bit for bit; the one launch (the DRIVE builds of the lane kernel) against the stepwise
form bit for bit; across the wave limit, with ragged leading dimensions, with cars no caller should send, and the refusals that need
a live handle."""
import ctypes as C
import os

import numpy as np
import pytest

import drive_helpers as D
from helpers import TOL_STEER

pytestmark = pytest.mark.gpu

F, I = D.SENTINEL, D.ISENTINEL


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return D.load_drive_twin()


def _t(a, dev, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _params(pkg, golden_dir, **over):
    return pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), N=10, **over)


def _drive(pkg, params, waypoints, car, steps, dev, host=False, fused=False, **kw):
    """mpc_drive_batch_device (fused: mpc_drive_batch_device_fused; host: mpc_drive_batch_host) through the raw ABI
    (drive_helpers.device_drive: ragged ld, NaN and sentinels behind column B)"""
    return D.device_drive(pkg, params, waypoints, car, steps, dev, form="host" if host else ("fused" if fused else "device"), entry="", **kw)


def _same(a, b, what=""):
    for k in ("car", "summary", "hist", "status", "iters"):
        if a[k] is not None and b[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.fixture(scope="module")
def loop96(pkg, golden_dir, waypoints, torch_dev):
    """B = 96 cars x 8 steps on the device, cold and warm, with the default wave limit (the wave kernels): computed once, shared."""
    params = _params(pkg, golden_dir)
    car = pkg.scenarios.track_starts(96, params, waypoints, seed=4)
    return params, car, {w: _drive(pkg, params, waypoints, car, 8, torch_dev, warm=w) for w in (0, 1)}


@pytest.mark.parametrize("warm", [0, 1])
def test_stepwise_against_the_cpu_build(pkg, twin, waypoints, loop96, warm):
    """Windows (row 12) and statuses equal at every step; cmd compared solve by solve -- the CPU build re-run on the device's recorded
    car and window -- so loop amplification cannot enter; the summary rows follow from the records."""
    params, car, res = loop96
    dev = res[warm]
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    tw = D.twin_drive(twin, params, waypoints, car, 8, opts, wopts)
    assert np.array_equal(dev["hist"][:, D.REC_K], tw["hist"][:, D.REC_K]) and np.array_equal(dev["hist"][:, D.REC_STATUS], tw["hist"][:, D.REC_STATUS])
    assert dev["info"] == {"fused_launches": 0, "stepwise_loops": 1}
    mem = {"warm": None, "status": None}
    d_steer = d_thr = 0.0
    for t in range(8):
        h = dev["hist"][t]
        assert np.array_equal(D.twin_window(twin, waypoints, h[0], h[1]), h[D.REC_K].astype(np.int32))
        r = D.twin_handler(twin, params, waypoints, h[:6], h[D.REC_K], opts, wopts, warm=mem["warm"] if warm else None,
                           warm_status=mem["status"] if warm else None, want_warm=bool(warm))
        mem["warm"], mem["status"] = r["warm"], r["status"]
        assert np.array_equal(r["status"], h[D.REC_STATUS].astype(np.int32)), t
        ok = r["status"] == 0
        d_steer = max(d_steer, (np.abs(r["cmd"][0] - h[D.REC_CMD])[ok] * params.max_steering).max())
        d_thr = max(d_thr, np.abs(r["cmd"][1] - h[D.REC_CMD + 1])[ok].max())
        assert np.abs(r["cte_epsi"] - h[D.REC_CTE:D.REC_EPSI + 1])[:, ok].max() <= 1e-9
    print("device vs CPU build, warm %d: max |d steer| %.3g rad, |d throttle| %.3g" % (warm, d_steer, d_thr))
    assert d_steer <= TOL_STEER and d_thr <= D.TOL_THROTTLE
    D.check_summary(dev, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("warm", [0, 1])
def test_every_step_is_the_handlers_own_answer(pkg, waypoints, loop96, torch_dev, warm):
    """mpc_telemetry_batch_device(_warm) on hist's car and window of step k returns bitwise hist's cmd and status (weights NULL)."""
    import torch
    params, car, res = loop96
    hist = res[warm]["hist"]
    B = car.shape[1]
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        wbuf = torch.empty((mpc.warm_rows(), B), dtype=torch.float64, device=torch_dev)
        status = torch.empty((B,), dtype=torch.int32, device=torch_dev)
        for t in range(hist.shape[0]):
            px, py = D.window_points(waypoints, hist[t, D.REC_K].astype(np.int64))
            kw = dict(warm=wbuf if t > 0 else None, warm_status=status if t > 0 else None, warm_out=wbuf, status_out=status) if warm else {}
            r = mpc.telemetry_torch(_t(hist[t, :6], torch_dev), _t(px, torch_dev), _t(py, torch_dev), **kw)
            torch.cuda.synchronize()
            assert np.array_equal(r["cmd"].cpu().numpy(), hist[t, D.REC_CMD:D.REC_CMD + 2]), t
            assert np.array_equal(r["status"].cpu().numpy(), hist[t, D.REC_STATUS].astype(np.int32)), t


@pytest.fixture(scope="module")
def cars200(pkg, golden_dir, waypoints):
    params = _params(pkg, golden_dir)
    return pkg.scenarios.track_starts(200, params, waypoints, seed=6), pkg.scenarios.weight_sweep(200, params, seed=91)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_lane_kernels_and_wave_kernels_write_the_same_bits(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """ld = B + 3, 5 steps and 1, with and without per-instance weights, hist NULL and not: wave_max_batch = -1 (every size reaches the
    lane kernel) against the default limit (the wave kernels, as the telemetry entry point dispatches) -- the same bits; hist = NULL
    changes nothing else; the first step of 5 is the call with steps = 1; per-instance weights reach the solve, and the handle's own
    weights as an array are the call without one."""
    car, weights = cars200[0][:, :B], cars200[1][:, :B]
    lane_p, wave_p = _params(pkg, golden_dir, wave_max_batch=-1), _params(pkg, golden_dir)
    for w in (None, weights):
        lane = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, warm=warm, weights=w)
        wave = _drive(pkg, wave_p, waypoints, car, 5, torch_dev, warm=warm, weights=w)
        _same(lane, wave, "lane / wave")
        assert lane["info"]["stepwise_loops"] == 1
        _same(lane, _drive(pkg, lane_p, waypoints, car, 5, torch_dev, warm=warm, weights=w, hist=False), "hist = NULL")
        one = _drive(pkg, lane_p, waypoints, car, 1, torch_dev, warm=warm, weights=w)
        assert np.array_equal(one["hist"][0], lane["hist"][0]) and np.array_equal(one["car"], lane["hist"][1, :6])
    plain = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, warm=warm)
    swept = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, warm=warm, weights=weights)
    if B >= 63:
        assert not np.array_equal(plain["hist"][:, D.REC_CMD], swept["hist"][:, D.REC_CMD])      # the weights reach the solve
    own = np.tile(np.array([lane_p.weights[i] for i in range(12)])[:, None], (1, B))
    _same(plain, _drive(pkg, lane_p, waypoints, car, 5, torch_dev, warm=warm, weights=own), "the handle's weights as an array")


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_fused_equals_stepwise_bitwise(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The one launch writes the stepwise form's bits into car, summary, hist, status and iters: ld = B + 3, steps 1 and 5, hist NULL
    and not, with and without per-instance weights, wave_max_batch = -1 so that every size reaches the lane kernel -- and
    mpc_drive_info says that the fused kernel ran."""
    car, weights = cars200[0][:, :B], cars200[1][:, :B]
    lane_p = _params(pkg, golden_dir, wave_max_batch=-1)
    for steps in (1, 5):
        for hist in (True, False):
            for w in (None, weights):
                a = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, warm=warm, weights=w, hist=hist)
                b = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, warm=warm, weights=w, hist=hist, fused=True)
                _same(a, b, "fused / stepwise, steps %d hist %s weights %s" % (steps, hist, w is not None))
                assert a["info"] == {"fused_launches": 0, "stepwise_loops": 1} and b["info"] == {"fused_launches": 1, "stepwise_loops": 0}


@pytest.mark.parametrize("warm", [0, 1])
def test_fused_call_below_the_wave_limit_runs_the_stepwise_loop(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """With the default wave limit and B = 65 the fused call runs the stepwise loop itself, says so, and the bits are still equal --
    to the stepwise call and to the one launch of a handle without the wave path."""
    car = cars200[0][:, :65]
    a = _drive(pkg, _params(pkg, golden_dir), waypoints, car, 5, torch_dev, warm=warm)
    b = _drive(pkg, _params(pkg, golden_dir), waypoints, car, 5, torch_dev, warm=warm, fused=True)
    c = _drive(pkg, _params(pkg, golden_dir, wave_max_batch=-1), waypoints, car, 5, torch_dev, warm=warm, fused=True)
    assert b["info"] == {"fused_launches": 0, "stepwise_loops": 1} and c["info"] == {"fused_launches": 1, "stepwise_loops": 0}
    _same(a, b, "fused call, wave path"); _same(a, c, "one launch against the wave kernels")


@pytest.mark.parametrize("wave_max_batch,fused", [(0, False), (-1, False), (-1, True)])
def test_containment(pkg, golden_dir, waypoints, torch_dev, wave_max_batch, fused):
    """One car with NaN x, one at speed -1 mph, one 1e6 m from the track: the launch ends, those cars carry a non-success status, and
    every other car is bitwise what it is in a batch without them.  Both forms (the stepwise one on the wave and on the lane kernels)."""
    params = _params(pkg, golden_dir, wave_max_batch=wave_max_batch)
    clean = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    dirty = clean.copy()
    bad = [5, 17, 70]
    dirty[0, 5] = np.nan; dirty[3, 17] = -1.0; dirty[0, 70] += 1e6
    for warm in (0, 1):
        a = _drive(pkg, params, waypoints, clean, 4, torch_dev, warm=warm, fused=fused)
        b = _drive(pkg, params, waypoints, dirty, 4, torch_dev, warm=warm, fused=fused)
        assert b["info"]["fused_launches"] == (1 if fused else 0)
        assert (b["status"][bad] != 0).all() and (b["summary"][7, bad] >= 1).all()
        good = np.setdiff1d(np.arange(80), bad)
        for k in ("car", "summary", "hist", "status", "iters"):
            assert np.array_equal(a[k][..., good], b[k][..., good]), k
        assert (a["status"] == 0).all()


def test_host_form(pkg, golden_dir, waypoints, cars200, torch_dev):
    params = _params(pkg, golden_dir)
    car, weights = cars200[0][:, :65], cars200[1][:, :65]
    for warm in (0, 1):
        _same(_drive(pkg, params, waypoints, car, 3, torch_dev, warm=warm, weights=weights),
              _drive(pkg, params, waypoints, car, 3, torch_dev, warm=warm, weights=weights, host=True), "host form")


def test_drive_torch(pkg, golden_dir, waypoints, loop96, torch_dev):
    import torch
    params, car, res = loop96
    tx, ty = D.track_of(waypoints)
    with pkg.BatchedMPC(params, 96, device=0) as mpc:
        r = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 8, opts=mpc.drive_opts(warm_start=1))
        torch.cuda.synchronize()
        for k in ("car", "summary", "hist", "status", "iters"):
            assert np.array_equal(r[k].cpu().numpy(), res[1][k]), k
        f = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 8, opts=mpc.drive_opts(warm_start=1), fused=True)
        torch.cuda.synchronize()
        for k in ("car", "summary", "hist", "status", "iters"):
            assert np.array_equal(f[k].cpu().numpy(), res[1][k]), k
        assert mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 2}       # (96 cars: below the wave limit)
        n = mpc.drive_numpy(car, tx, ty, 8, opts=mpc.drive_opts(warm_start=1))
        for k in ("car", "summary", "hist", "status", "iters"):
            assert np.array_equal(n[k], res[1][k]), k


def test_refusals_on_a_live_handle(pkg, golden_dir, waypoints, torch_dev):
    import torch
    lib = pkg.library()
    tx, ty = D.track_of(waypoints)
    B = 8
    params = _params(pkg, golden_dir)
    car = _t(pkg.scenarios.track_starts(B, params, waypoints), torch_dev)
    d_tx, d_ty = _t(tx, torch_dev), _t(ty, torch_dev)
    summ = torch.full((8, B), F, dtype=torch.float64, device=torch_dev); st = torch.full((B,), I, dtype=torch.int32, device=torch_dev)
    before = car.clone()

    def call(h, opts, B_=B, ld=B, steps=2, car_=car, tx_=d_tx, n=len(tx), summ_=summ, st_=st):
        p = lambda t: t.data_ptr() if t is not None else None
        return lib.mpc_drive_batch_device(h, B_, ld, steps, p(car_), p(tx_), p(d_ty), n, None, C.byref(opts), None, p(summ_), None, p(st_), None, None)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        good = mpc.drive_opts()
        o = lambda **k: mpc.drive_opts(**k)
        for args, kw, text in (((o(size=8),), {}, b"size"), ((good,), dict(steps=0), b"steps"), ((o(npts=2),), {}, b"npts"), ((o(npts=9),), {}, b"npts"),
                               ((good,), dict(n=5), b"n_track"), ((good,), dict(n=4097), b"n_track"), ((o(sub_old=-1),), {}, b"substep"),
                               ((o(sub_old=0, sub_new=0),), {}, b"sub_old"), ((o(sub_old=999, sub_new=2),), {}, b"sub_old"), ((o(h=0.0),), {}, b"h must"),
                               ((o(h=float("nan")),), {}, b"h must"), ((o(h=float("inf")),), {}, b"h must"), ((good,), dict(ld=B - 1), b"ld"),
                               ((good,), dict(car_=None), b"NULL"), ((good,), dict(tx_=None), b"NULL"), ((good,), dict(summ_=None), b"NULL"),
                               ((good,), dict(st_=None), b"NULL")):
            rc = call(mpc._h, *args, **kw)
            assert rc == -1 and text in lib.mpc_last_error(), (rc, text, lib.mpc_last_error())
        assert mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
        torch.cuda.synchronize()
        assert torch.equal(car, before) and (summ == F).all() and (st == I).all()      # a refused call touches nothing
    with pkg.BatchedMPC(_params(pkg, golden_dir, precision=pkg.PRECISION_F32), B, device=0) as mpc:
        assert call(mpc._h, good) == -1 and b"fp64" in lib.mpc_last_error()
    with pkg.BatchedMPC(_params(pkg, golden_dir, max_soc=4), B, device=0) as mpc:
        assert call(mpc._h, pkg.drive_opts_default(params, warm_start=1)) == -4 and b"second-order" in lib.mpc_last_error()
        assert call(mpc._h, good) == 0                                     # cold with SOC: served
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all()
    assert not torch.equal(car, before)
