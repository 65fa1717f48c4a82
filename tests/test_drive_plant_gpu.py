"""Track driving with per-car plant values on the device (mpc_drive_batch_device_plant / _fused_plant / _host_plant;
include/mpc_amd_drive.h): plant = NULL against the _horizon forms; the default column against plant = NULL; a mixed batch against its
uniform parts; the one launch against the stepwise form bit for bit, across the wave limit and with ragged leading dimensions; the lane
kernels against the wave kernels; the stepwise form against the CPU build (tests/drive_twin) step by step; unusable columns; the
host form, the Python layer and the refusals that need a live handle."""
import ctypes as C
import itertools

import numpy as np
import pytest

import drive_helpers as D
import drive_latency_helpers as DL
import drive_plant_helpers as DP
from drive_horizon_helpers import mixed_horizons
from drive_helpers import fast_params as _params, to_device as _t
from helpers import TOL_STEER
from model_helpers import draw_rows
from run_model_helpers import uniform_model

pytestmark = pytest.mark.gpu

F, I = D.SENTINEL, D.ISENTINEL
_drive, _same = DP.device_drive, DP.same
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
    """cars, weights, model, latency, plant, horizon of 200 cars: drawn once, never changed"""
    params = _params(pkg, golden_dir)
    return (pkg.scenarios.track_starts(200, params, waypoints, seed=6), pkg.scenarios.weight_sweep(200, params, seed=91),
            draw_rows(params, 200, seed=9), DL.draw_latency(200), DP.draw_plant(200), mixed_horizons(200))


@pytest.mark.parametrize("warm", [0, 1])
def test_plant_null_is_the_horizon_form(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """B = 65, all three forms, the wave kernels and the lane kernels, without and with model / latency / horizon: bitwise, and the same
    mpc_drive_info."""
    car, weights, model, lat, _, hz = (a[..., :65] for a in cars200)
    for params in (_params(pkg, golden_dir), _params(pkg, golden_dir, wave_max_batch=-1)):
        for form in ("device", "fused", "host"):
            for m, l, z in ((None, None, None), (model, lat, None), (model, lat, hz)):
                a = _drive(pkg, params, waypoints, car, 2, torch_dev, model=m, horizon=z, latency=l, plant=None, form=form, warm=warm, weights=weights)
                b = _drive(pkg, params, waypoints, car, 2, torch_dev, model=m, horizon=z, latency=l, form=form, entry="horizon", warm=warm, weights=weights)
                _same(a, b)
                assert a["info"] == b["info"], (form, m is not None, z is not None)


@pytest.mark.parametrize("warm", [0, 1])
def test_default_column_is_plant_null(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """The default column (row 0: the model's Lf with a model, the handle's without) is bitwise the plant = NULL call: the stepwise loop
    on the wave kernels and the one launch."""
    car, model = cars200[0][:, :65], cars200[2][:, :65]
    for wave, form, info in ((0, "device", STEPWISE), (-1, "fused", ONE_LAUNCH)):
        params = _params(pkg, golden_dir, wave_max_batch=wave)
        for m in (None, model):
            plant = pkg.drive_plant_default(params, 65, m)
            assert np.array_equal(plant[0], model[1] if m is not None else np.full(65, params.Lf))
            a = _drive(pkg, params, waypoints, car, 4, torch_dev, model=m, plant=plant, form=form, warm=warm)
            b = _drive(pkg, params, waypoints, car, 4, torch_dev, model=m, plant=None, form=form, warm=warm)
            _same(a, b)
            assert a["info"] == b["info"] == info


GROUPS = ((2.0, 1.0, 0.0, 6.0, 50.0, 0.0), (2.67, 0.8, 0.03, 6.0, 50.0, 0.0), (3.5, 1.2, -0.02, 4.0, 70.0, 0.5), (2.67, 1.0, 0.0, 8.0, 40.0, -1.0))


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("form,wave", [("device", 0), ("fused", -1)])
def test_a_mixed_batch_is_its_uniform_parts(pkg, golden_dir, waypoints, cars200, torch_dev, warm, form, wave):
    """B = 200 cars in 4 interleaved groups with 4 different columns: car i of the mixed call is bitwise car i of a call with its
    group's column uniform, and the cars of the other groups differ.  5 steps; the stepwise loop on the wave kernels and the one
    launch."""
    car, weights = cars200[0], cars200[1]
    params = _params(pkg, golden_dir, wave_max_batch=wave)
    g_of = np.arange(200) % 4
    plant = np.ascontiguousarray(np.array([[GROUPS[g][r] for g in g_of] for r in range(6)], dtype=np.float64))
    mixed = _drive(pkg, params, waypoints, car, 5, torch_dev, plant=plant, form=form, warm=warm, weights=weights)
    assert mixed["info"] == (ONE_LAUNCH if form == "fused" else STEPWISE)
    for g, col in enumerate(GROUPS):
        ref = _drive(pkg, params, waypoints, car, 5, torch_dev, plant=DP.uniform_plant(200, col), form=form, warm=warm, weights=weights)
        _same(mixed, ref, cars=np.nonzero(g_of == g)[0])
        others = np.nonzero(g_of != g)[0]
        assert (mixed["car"][0, others] != ref["car"][0, others]).all()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_fused_equals_stepwise_bitwise(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The one launch writes the stepwise plant loop's bits: ld = B + 3, steps 1 and 5, hist NULL and not, with and without model,
    weights and latency (the pairings of tests/test_drive_latency_gpu.py over the four (steps, hist) cases), once more with a horizon,
    wave_max_batch = -1 so that every size reaches the lane kernel -- and mpc_drive_info says which ran.  The columns reach the drive:
    the results differ from plant = NULL."""
    car, weights, model, lat, plant, hz = (a[..., :B] for a in cars200)
    lane_p = _params(pkg, golden_dir, wave_max_batch=-1)
    pairs = [(None, None, lat), (model, weights, lat), (model, None, None), (None, weights, None)]
    for (steps, hist), (m, w, l) in zip(itertools.product((1, 5), (True, False)), pairs):
        a = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, model=m, latency=l, plant=plant, warm=warm, weights=w, hist=hist)
        b = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, model=m, latency=l, plant=plant, warm=warm, weights=w, hist=hist, form="fused")
        _same(a, b)
        assert a["info"] == STEPWISE and b["info"] == ONE_LAUNCH, (steps, hist)
    u = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, plant=None, warm=warm, weights=weights, hist=False, form="fused")
    assert not np.array_equal(u["car"], b["car"])
    a = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, model=model, horizon=hz, latency=lat, plant=plant, warm=warm)
    b = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, model=model, horizon=hz, latency=lat, plant=plant, warm=warm, form="fused")
    _same(a, b)
    assert a["info"] == STEPWISE and b["info"] == ONE_LAUNCH


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("warm", [0, 1])
def test_lane_kernels_and_wave_kernels_write_the_same_bits(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The stepwise plant loop with wave_max_batch = -1 (the lane kernel) against the default limit (the wave kernel): ld = B + 3,
    5 steps, with model, weights and latency and without -- the same bits; hist = NULL changes nothing else."""
    car, weights, model, lat, plant, _ = (a[..., :B] for a in cars200)
    lane_p, wave_p = _params(pkg, golden_dir, wave_max_batch=-1), _params(pkg, golden_dir)
    for m, w, l in ((None, None, None), (model, weights, lat)):
        lane = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, model=m, latency=l, plant=plant, warm=warm, weights=w)
        _same(lane, _drive(pkg, wave_p, waypoints, car, 5, torch_dev, model=m, latency=l, plant=plant, warm=warm, weights=w))
        _same(lane, _drive(pkg, lane_p, waypoints, car, 5, torch_dev, model=m, latency=l, plant=plant, warm=warm, weights=w, hist=False))
        assert lane["info"] == STEPWISE


@pytest.mark.parametrize("warm", [0, 1])
def test_stepwise_against_the_cpu_build(pkg, twin, golden_dir, waypoints, torch_dev, warm):
    """B = 65 cars x 5 messages with the columns draw_latency and draw_plant.  Windows and statuses equal at every step; the replies
    compared solve by solve -- the CPU build's handler re-run on the device's recorded car and window with the car's comp -- within the
    bounds of tests/test_drive_latency_gpu.py::test_stepwise_against_the_cpu_build; the cars after every plant step against the CPU
    build's plant with the car's own column and counts, 4 x its substeps ulp, as there."""
    params = _params(pkg, golden_dir)
    B, steps = 65, 5
    car = pkg.scenarios.track_starts(B, params, waypoints, seed=4)
    lat, plant = DL.draw_latency(B, seed=23), DP.draw_plant(B, seed=33)
    dev = _drive(pkg, params, waypoints, car, steps, torch_dev, latency=lat, plant=plant, warm=warm)
    assert dev["info"] == STEPWISE
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    model = uniform_model(params, B)
    tw = DP.twin_drive_plant(twin, params, waypoints, car, model, lat, plant, steps, opts, wopts)
    assert np.array_equal(dev["hist"][:, D.REC_K], tw["hist"][:, D.REC_K]) and np.array_equal(dev["hist"][:, D.REC_STATUS], tw["hist"][:, D.REC_STATUS])
    mem = {"warm": None, "status": None}
    d_steer = d_thr = 0.0
    for t in range(steps):
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
        nxt = dev["hist"][t + 1, :6] if t < steps - 1 else dev["car"]
        ref = np.empty((6, B))
        for i in range(B):
            ref[:, i:i + 1] = DP.twin_plant(twin, params, h[:6, i:i + 1], h[D.REC_CMD:D.REC_CMD + 2, i:i + 1], model[:, i:i + 1], plant[:, i:i + 1],
                                            int(lat[DL.SUB_OLD, i]), int(lat[DL.SUB_NEW, i]), opts.h)[0]
        assert (np.abs(nxt - ref) <= 4 * (lat[DL.SUB_OLD] + lat[DL.SUB_NEW])[None, :] * np.spacing(np.maximum(1.0, np.abs(ref)))).all(), t
        assert np.array_equal(nxt[4], h[D.REC_CMD] * params.max_steering) and np.array_equal(nxt[5], h[D.REC_CMD + 1])
    print("device vs CPU build, warm %d: max |d steer| %.3g rad, |d throttle| %.3g; statuses %s" % (
        warm, d_steer, d_thr, np.bincount(dev["hist"][:, D.REC_STATUS].astype(np.int64).ravel())))
    assert d_steer <= TOL_STEER and d_thr <= D.TOL_THROTTLE
    D.check_summary(dev, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("wave_max_batch,fused", [(0, False), (-1, False), (-1, True)])
def test_unusable_columns(pkg, golden_dir, waypoints, torch_dev, wave_max_batch, fused):
    """Not-a-number and infinity in each row, Lf_p = 0 and -1, d = 0 in 15 of 80 cars (drive_plant_helpers.unusable_case).  Each such car
    is moved with the default column and every step the handler ended SUCCESS or ACCEPTABLE is INFEASIBLE in hist row 10, summary row 7
    and the folded status; nothing is not-a-number; the iterations are those of the car under the default column, and so -- warm -- is
    every later step: the next step is still warm-started.  Every other car is bitwise the batch without the defect.  The drives run
    in a child process under a time limit of its own."""
    res = D.run_in_child("drive_plant_helpers.child_runs", fused, wave_max_batch)
    params = _params(pkg, golden_dir, wave_max_batch=wave_max_batch)
    car, plant, dirty, bad = DP.unusable_case(pkg, params, waypoints)
    ref_plant = plant.copy(); ref_plant[:, bad] = pkg.drive_plant_default(params)[:, None]
    good = np.setdiff1d(np.arange(80), bad)
    other = [r for r in range(D.REC) if r != D.REC_STATUS]
    for warm in (0, 1):
        a, b = res[warm, "clean"], res[warm, "dirty"]
        assert b["info"] == (ONE_LAUNCH if fused else STEPWISE)
        _same(a, b, cars=good)
        for k in ("car", "summary", "hist"):
            assert np.isfinite(b[k]).all(), k
        # the same cars under the default column: the handler's own statuses, and every bit but the status rows
        ref = _drive(pkg, params, waypoints, car, 4, torch_dev, plant=ref_plant, warm=warm, form="fused" if fused else "device")
        want = DP.expected_status(ref["hist"][:, D.REC_STATUS][:, bad].astype(np.int32))
        assert (ref["hist"][:, D.REC_STATUS][:, bad] == 0).mean() > 0.8
        assert np.array_equal(b["hist"][:, D.REC_STATUS][:, bad].astype(np.int32), want) and (want != 0).all()
        assert (b["summary"][7, bad] == 4).all() and np.array_equal(b["status"][bad], want.max(0))
        assert np.array_equal(b["iters"], ref["iters"]) and np.array_equal(b["hist"][:, other], ref["hist"][:, other])
        assert np.array_equal(b["car"], ref["car"]) and np.array_equal(b["summary"][:7], ref["summary"][:7])
    # (warm is not cold: the equality above says something about the warm rule)
    assert not np.array_equal(res[0, "dirty"]["hist"][1:, D.REC_ITERS][:, bad], res[1, "dirty"]["hist"][1:, D.REC_ITERS][:, bad])


def test_host_form_and_python_layer(pkg, golden_dir, waypoints, cars200, torch_dev):
    """_host_plant is bitwise the device form at B = 7; drive_torch(plant=...) and drive_numpy(plant=...) give the same results, with
    and without the other arrays; shape and dtype errors raise ValueError."""
    import torch
    params = _params(pkg, golden_dir)
    car, weights, model, lat, plant, hz = (a[..., :7] for a in cars200)
    tx, ty = D.track_of(waypoints)
    for warm in (0, 1):
        dev = _drive(pkg, params, waypoints, car, 3, torch_dev, model=model, latency=lat, plant=plant, warm=warm, weights=weights)
        _same(dev, _drive(pkg, params, waypoints, car, 3, torch_dev, model=model, latency=lat, plant=plant, warm=warm, weights=weights, form="host"))
        alone = _drive(pkg, params, waypoints, car, 3, torch_dev, plant=plant, warm=warm)
        _same(alone, _drive(pkg, params, waypoints, car, 3, torch_dev, plant=plant, warm=warm, form="host"))
        full = _drive(pkg, params, waypoints, car, 3, torch_dev, model=model, horizon=hz, latency=lat, plant=plant, warm=warm)
        _same(full, _drive(pkg, params, waypoints, car, 3, torch_dev, model=model, horizon=hz, latency=lat, plant=plant, warm=warm, form="host"))
        with pkg.BatchedMPC(params, 7, device=0) as mpc:
            o = mpc.drive_opts(warm_start=warm)
            for fused in (False, True):
                r = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, weights=_t(weights, torch_dev), opts=o, fused=fused,
                                    model=_t(model, torch_dev), latency=_t(lat, torch_dev), plant=_t(plant, torch_dev))
                torch.cuda.synchronize()
                for k in DP.KEYS:
                    assert np.array_equal(r[k].cpu().numpy(), dev[k]), (k, fused)
            _same(mpc.drive_numpy(car, tx, ty, 3, weights=weights, opts=o, model=model, latency=lat, plant=plant), dev)
            _same(mpc.drive_numpy(car, tx, ty, 3, opts=o, plant=plant), alone)
            _same(mpc.drive_numpy(car, tx, ty, 3, opts=o, model=model, horizon=hz, latency=lat, plant=plant), full)
            assert np.array_equal(mpc.drive_plant_default(), pkg.drive_plant_default(params))
            _same(mpc.drive_numpy(car, tx, ty, 3, opts=o, model=model, plant=mpc.drive_plant_default(7, model)), mpc.drive_numpy(car, tx, ty, 3, opts=o, model=model))
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, plant=_t(plant[:, :6], torch_dev))
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, plant=_t(plant, torch_dev).float())
            with pytest.raises(ValueError):
                mpc.drive_numpy(car, tx, ty, 3, plant=plant[:5])


def test_refusals_on_a_live_handle(pkg, golden_dir, waypoints, torch_dev):
    """With a plant array an F32 handle is refused first (MPC_ERR_INVALID, the fp64-handles-only text of the drive), before what the
    _horizon forms refuse: warm_start with max_soc > 0: MPC_ERR_UNSUPPORTED; a horizon with max_soc > 0: MPC_ERR_UNSUPPORTED; ld < B and
    a bad count: MPC_ERR_INVALID.  A refused call touches nothing."""
    import torch
    lib = pkg.library()
    tx, ty = D.track_of(waypoints)
    B = 8
    params = _params(pkg, golden_dir)
    car = _t(pkg.scenarios.track_starts(B, params, waypoints), torch_dev)
    plant = _t(DP.draw_plant(B), torch_dev)
    hz = _t(mixed_horizons(B), torch_dev, np.int32)
    d_tx, d_ty = _t(tx, torch_dev), _t(ty, torch_dev)
    summ = torch.full((8, B), F, dtype=torch.float64, device=torch_dev); st = torch.full((B,), I, dtype=torch.int32, device=torch_dev)
    before = car.clone()
    names = ("mpc_drive_batch_device_plant", "mpc_drive_batch_device_fused_plant")

    def drive(h, opts, name, ld=B, horizon=None, model=None):
        return getattr(lib, name)(h, B, ld, 2, car.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(), len(tx), None, model, horizon, None, plant.data_ptr(),
                                  C.byref(opts), None, summ.data_ptr(), None, st.data_ptr(), None, None)

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(car, before) and bool((summ == F).all()) and bool((st == I).all())
    good = pkg.drive_opts_default(params)
    with pkg.BatchedMPC(_params(pkg, golden_dir, precision=pkg.PRECISION_F32), B, device=0) as mpc:
        for name in names:
            assert drive(mpc._h, good, name) == -1 and b"track driving: fp64 handles only" in lib.mpc_last_error()
            # ... first: also where the horizon rule has a text of its own for such a handle
            assert drive(mpc._h, good, name, horizon=hz.data_ptr()) == -1 and b"track driving: fp64 handles only" in lib.mpc_last_error()
        assert untouched() and mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        for name in names:
            assert drive(mpc._h, good, name, ld=B - 1) == -1 and b"ld" in lib.mpc_last_error()
            bad = pkg.drive_opts_default(params, sub_old=-1)
            assert drive(mpc._h, bad, name) == -1 and b"substep" in lib.mpc_last_error()
        assert untouched() and mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
    with pkg.BatchedMPC(_params(pkg, golden_dir, max_soc=4), B, device=0) as mpc:
        for name in names:
            assert drive(mpc._h, pkg.drive_opts_default(params, warm_start=1), name) == -4 and b"second-order" in lib.mpc_last_error()
            assert drive(mpc._h, good, name, horizon=hz.data_ptr()) == -4 and b"second-order" in lib.mpc_last_error()
        assert untouched()
        assert drive(mpc._h, good, "mpc_drive_batch_device_fused_plant") == 0          # cold with SOC: served, by the stepwise loop
        torch.cuda.synchronize()
        assert (st.cpu().numpy() != I).all() and mpc.drive_info() == STEPWISE
