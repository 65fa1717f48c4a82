"""The track drive under noise on the device (mpc_drive_batch_device_noise / _fused_noise / _host_noise; include/mpc_amd_noise.h):
noise = NULL and seen = NULL against the _budget forms; the zero column against NULL; the one launch against the stepwise form bit for
bit, seen included, across the wave limit and with ragged leading dimensions; the lane kernels against the wave kernels; a mixed batch
against its uniform parts and its own reversal; the draw function on the device against its host evaluation; the stepwise form against
the CPU build (tests/drive_twin/noise_drive_twin.cpp) step by step; columns that cannot be used; the host form, the Python layer and
the refusals that need a live handle.  config-fast.json at N = 10; cars from scenarios.track_starts(200), columns drawn once."""
import ctypes as C
import itertools

import numpy as np
import pytest

import drive_helpers as D
import drive_latency_helpers as DL
import drive_plant_helpers as DP
import noise_helpers as NH
from drive_helpers import fast_params as _params, to_device as _t
from drive_horizon_helpers import mixed_horizons
from helpers import TOL_STEER
from model_helpers import draw_rows
from noise_helpers import device_noise_drive as _drive, same as _same

pytestmark = pytest.mark.gpu

F, I = NH.SENTINEL, NH.ISENTINEL
ONE_LAUNCH, STEPWISE = {"fused_launches": 1, "stepwise_loops": 0}, {"fused_launches": 0, "stepwise_loops": 1}
SIZES = [1, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return NH.load_noise_drive_twin()


@pytest.fixture(scope="module")
def cars200(pkg, golden_dir, waypoints):
    """cars, weights, model, latency, plant, horizon, budget, noise of 200 cars: drawn once, never changed"""
    params = _params(pkg, golden_dir)
    budget = np.array([(4, 8, 50, 50)[i % 4] for i in range(200)], dtype=np.int32)
    return (pkg.scenarios.track_starts(200, params, waypoints, seed=6), pkg.scenarios.weight_sweep(200, params, seed=91), draw_rows(params, 200, seed=9),
            DL.draw_latency(200), DP.draw_plant(200), mixed_horizons(200), budget, NH.noise_columns(200))


@pytest.mark.parametrize("warm", [0, 1])
def test_null_noise_and_null_seen_is_the_budget_form(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """B = 65, 2 steps, all three forms, the wave kernels and the lane kernels, without and with model / latency / horizon / plant /
    budget: bitwise, and the same mpc_drive_info."""
    car, weights, model, lat, plant, hz, budget, _ = (a[..., :65] for a in cars200)
    for params in (_params(pkg, golden_dir), _params(pkg, golden_dir, wave_max_batch=-1)):
        for form in ("device", "fused", "host"):
            for kw in ({}, dict(model=model, latency=lat, plant=plant), dict(model=model, latency=lat, plant=plant, horizon=hz, budget=budget)):
                a = _drive(pkg, params, waypoints, car, 2, torch_dev, noise=None, seen=False, form=form, warm=warm, weights=weights, **kw)
                b = _drive(pkg, params, waypoints, car, 2, torch_dev, seen=False, form=form, entry="budget", warm=warm, weights=weights, **kw)
                _same(a, b)
                assert a["info"] == b["info"], (form, sorted(kw))


@pytest.mark.parametrize("warm", [0, 1])
def test_zero_column_is_null(pkg, golden_dir, waypoints, cars200, torch_dev, warm):
    """B = 65, 4 steps: the zero column (with the cars' seeds in it) is bitwise the noise = NULL call, which with `seen` given is the
    call without and writes the true cars there: the stepwise loop on the wave kernels and the one launch."""
    car = cars200[0][:, :65]
    zero = NH.noise_columns(65, {})
    for wave, form, info in ((0, "device", STEPWISE), (-1, "fused", ONE_LAUNCH)):
        params = _params(pkg, golden_dir, wave_max_batch=wave)
        a = _drive(pkg, params, waypoints, car, 4, torch_dev, noise=zero, form=form, warm=warm)
        b = _drive(pkg, params, waypoints, car, 4, torch_dev, noise=None, form=form, warm=warm)
        c = _drive(pkg, params, waypoints, car, 4, torch_dev, noise=None, seen=False, form=form, warm=warm)
        _same(a, b)
        _same(b, c)
        assert np.array_equal(b["seen"], b["hist"][:, 0:4])
        assert a["info"] == b["info"] == c["info"] == info


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("warm", [0, 1])
def test_fused_equals_stepwise_bitwise(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The one launch writes the stepwise noisy loop's bits, seen included: ld = B + 3, steps 1 and 5, hist / seen given or NULL in the
    four pairings of tests/test_drive_plant_gpu.py (with and without model, weights and latency), once more with model + horizon +
    latency + plant + budget all present; wave_max_batch = -1 so that every size reaches the lane kernel -- and mpc_drive_info says
    which ran.  The noise reaches the drive: the results differ from noise = NULL."""
    car, weights, model, lat, plant, hz, budget, nz = (a[..., :B] for a in cars200)
    lane_p = _params(pkg, golden_dir, wave_max_batch=-1)
    pairs = [(None, None, lat), (model, weights, lat), (model, None, None), (None, weights, None)]
    for (steps, hist), (m, w, l) in zip(itertools.product((1, 5), (True, False)), pairs):
        kw = dict(model=m, latency=l, noise=nz, warm=warm, weights=w, hist=hist, seen=hist)
        a = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, **kw)
        b = _drive(pkg, lane_p, waypoints, car, steps, torch_dev, form="fused", **kw)
        _same(a, b)
        assert a["info"] == STEPWISE and b["info"] == ONE_LAUNCH, (steps, hist)
    u = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, noise=None, warm=warm, weights=weights, hist=False, seen=False, form="fused")
    assert not np.array_equal(u["car"], b["car"])
    for hist, seen in ((True, False), (False, True), (True, True)):
        kw = dict(model=model, horizon=hz, budget=budget, latency=lat, plant=plant, noise=nz, warm=warm, hist=hist, seen=seen)
        a = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, **kw)
        b = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, form="fused", **kw)
        _same(a, b)
        assert a["info"] == STEPWISE and b["info"] == ONE_LAUNCH


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("warm", [0, 1])
def test_lane_kernels_and_wave_kernels_write_the_same_bits(pkg, golden_dir, waypoints, cars200, torch_dev, B, warm):
    """The stepwise noisy loop with wave_max_batch = -1 (the lane kernel) against the default limit (the wave kernel): ld = B + 3,
    5 steps, with model, weights and latency and without -- the same bits, seen included."""
    car, weights, model, lat, _, _, _, nz = (a[..., :B] for a in cars200)
    lane_p, wave_p = _params(pkg, golden_dir, wave_max_batch=-1), _params(pkg, golden_dir)
    for m, w, l in ((None, None, None), (model, weights, lat)):
        lane = _drive(pkg, lane_p, waypoints, car, 5, torch_dev, model=m, latency=l, noise=nz, warm=warm, weights=w)
        _same(lane, _drive(pkg, wave_p, waypoints, car, 5, torch_dev, model=m, latency=l, noise=nz, warm=warm, weights=w))
        assert lane["info"] == STEPWISE


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("form,wave", [("device", 0), ("fused", -1)])
def test_a_mixed_batch_is_its_uniform_parts(pkg, golden_dir, waypoints, cars200, torch_dev, warm, form, wave):
    """B = 200 cars in 4 interleaved groups of different sigma rows (noise_helpers.GROUPS; every car keeps its seed): car i of the
    mixed call is bitwise car i of the call with its group's sigma rows uniform; the batch in reversed order gives the reversed
    outputs bitwise (nothing depends on the index).  5 steps; the stepwise loop on the wave kernels and the one launch."""
    car, weights = cars200[0], cars200[1]
    params = _params(pkg, golden_dir, wave_max_batch=wave)
    g_of = np.arange(200) % 4
    nz = NH.mixed_columns(200)
    mixed = _drive(pkg, params, waypoints, car, 5, torch_dev, noise=nz, form=form, warm=warm, weights=weights)
    assert mixed["info"] == (ONE_LAUNCH if form == "fused" else STEPWISE)
    for g, rows in enumerate(NH.GROUPS):
        ref = _drive(pkg, params, waypoints, car, 5, torch_dev, noise=NH.noise_columns(200, rows), form=form, warm=warm, weights=weights)
        _same(mixed, ref, cars=np.nonzero(g_of == g)[0])
        others = np.nonzero(g_of != g)[0]
        assert (mixed["car"][0, others] != ref["car"][0, others]).mean() > 0.9
    rev = np.arange(199, -1, -1)
    back = _drive(pkg, params, waypoints, np.ascontiguousarray(car[:, rev]), 5, torch_dev, noise=np.ascontiguousarray(nz[:, rev]), form=form, warm=warm,
                  weights=np.ascontiguousarray(weights[:, rev]))
    for k in NH.KEYS:
        assert np.ascontiguousarray(back[k][..., rev]).tobytes() == mixed[k].tobytes(), k


def test_device_draws(pkg, golden_dir, torch_dev):
    """mpc_debug_drive_noise_device on the stated 65 544 (seed, step) pairs against mpc_drive_noise_draw: u_drop bitwise, the normals
    within twice the bound of tests/test_drive_noise.py::test_draw_against_numpy, rad * 2 * noise_helpers.DRAW_REL -- both sides carry
    the library's share of it, and the device's square root is given the ulp numpy's functions were.  Pairs a column may not hold
    give not-a-number."""
    seed, step = NH.stated_pairs()
    host = NH.lib_draws(pkg.library(), seed, step)
    _, rad = NH.np_draw(seed.astype(np.uint64), step)
    with pkg.BatchedMPC(_params(pkg, golden_dir), 8, device=0) as mpc:
        dev = NH.device_draws(pkg, mpc, torch_dev, seed, step)
        bad = NH.device_draws(pkg, mpc, torch_dev, np.array([0.5, -1.0, 2.0 ** 53, np.nan, 7.0, 7.0]), np.array([0, 0, 0, 0, -1, 3], dtype=np.int32))
    assert np.isnan(bad[:, :5]).all() and np.isfinite(bad[:, 5]).all()
    assert np.array_equal(dev[6], host[6])
    err = np.abs(dev[:6] - host[:6])
    print("device draws: max |z_dev - z_host| / (rad * 2 DRAW_REL) = %.3f; bitwise equal in %.1f %%" % (
        (err / (rad[:6] * 2 * NH.DRAW_REL)).max(), 100.0 * (dev[:6] == host[:6]).mean()))
    assert (err <= rad[:6] * 2 * NH.DRAW_REL).all()


@pytest.mark.parametrize("warm", [0, 1])
def test_stepwise_against_the_cpu_build(pkg, twin, golden_dir, waypoints, torch_dev, warm):
    """B = 65 cars x 5 messages, all seven rows non-zero at moderate values (0.3 m, 0.02 rad, 1 mph, 0.01 rad, 0.3 m/s, 0.1).
    Windows and statuses equal the CPU build's at every step.  seen, A DEVIATION FROM THE ISSUE'S WORDING, which asks for the device's
    seen within the draw bound times sigma of the twin's at every step: that holds only while both sides hold the same true cars, and
    from the second message on they do not -- the replies may differ by TOL_STEER, the plant by ulps -- so a car-against-car comparison
    there would measure the drives' divergence, not the draw.  What is asserted instead asks no less of the draw: at the first message, where both sides hold the same cars,
    within the draw bound times sigma of the twin's (2 * DRAW_REL * rad * sigma, both sides carry the bound, plus an ulp of the sum
    each); at every message -- the two drives' cars part by what the replies may differ, so later messages are not compared car against
    car -- within the same bound of the device's own recorded car plus sigma * z with z from mpc_drive_noise_draw.  The replies solve by
    solve: the CPU build's handler re-run on the device's recorded seen and window, within the bounds of
    tests/test_drive_plant_gpu.py::test_stepwise_against_the_cpu_build (TOL_STEER, TOL_THROTTLE).  The cars after each plant step
    against the CPU build's plant under the perturbed column (bias and drift rebuilt from mpc_drive_noise_draw), 4 x substeps ulp as
    there.  Dropped messages, identified from u_drop, leave rows 4 / 5 unchanged."""
    params = _params(pkg, golden_dir)
    B, steps = 65, 5
    car = pkg.scenarios.track_starts(B, params, waypoints, seed=4)
    nz = NH.noise_columns(B)
    dev = _drive(pkg, params, waypoints, car, steps, torch_dev, noise=nz, warm=warm)
    assert dev["info"] == STEPWISE
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    tw = NH.twin_noise_drive(twin, params, waypoints, car, steps, opts, wopts, nz)
    assert np.array_equal(dev["hist"][:, D.REC_K], tw["hist"][:, D.REC_K]) and np.array_equal(dev["hist"][:, D.REC_STATUS], tw["hist"][:, D.REC_STATUS])
    z = np.array([[pkg.drive_noise_draw(s, t) for s in nz[NH.SEED]] for t in range(steps)]).transpose(0, 2, 1)      # [steps, 7, B]
    _, rad = NH.np_draw(np.tile(nz[NH.SEED].astype(np.uint64), steps), np.repeat(np.arange(steps), B))
    rad = rad.reshape(7, steps, B).transpose(1, 0, 2)
    sig = np.stack([nz[NH.POS], nz[NH.POS], nz[NH.PSI], nz[NH.SPEED]])
    tol = 2 * NH.DRAW_REL * rad[:, 0:4] * sig[None] + 2 * np.spacing(np.abs(dev["seen"]))
    assert (np.abs(dev["seen"][0] - tw["seen"][0]) <= tol[0]).all()
    rebuilt = dev["hist"][:, 0:4] + sig[None] * z[:, 0:4]
    rebuilt[:, 3] = np.maximum(0.0, rebuilt[:, 3])
    print("seen: max |device - (car + sigma z)| / bound = %.3f" % (np.abs(dev["seen"] - rebuilt) / tol).max())
    assert (np.abs(dev["seen"] - rebuilt) <= tol).all()
    dropped = z[:, NH.U_DROP] < nz[NH.DROP]
    assert dropped.any()
    dt = D.load_drive_twin()
    base = pkg.drive_plant_default(params, B)
    subs = opts.sub_old + opts.sub_new
    mem = {"warm": None, "status": None}
    d_steer = d_thr = 0.0
    for t in range(steps):
        h = dev["hist"][t]
        assert np.array_equal(D.twin_window(dt, waypoints, h[0], h[1]), h[D.REC_K].astype(np.int32))      # the window of the TRUE car
        told = np.concatenate([dev["seen"][t], h[4:6]])
        r = NH.twin_noise_handler(twin, params, waypoints, told, h[D.REC_K], opts, wopts, warm=mem["warm"] if warm else None,
                                  warm_status=mem["status"] if warm else None, want_warm=bool(warm))
        mem["warm"], mem["status"] = r["warm"], r["status"]
        assert np.array_equal(r["status"], h[D.REC_STATUS].astype(np.int32)), t
        ok = r["status"] == 0
        d_steer = max(d_steer, (np.abs(r["cmd"][0] - h[D.REC_CMD]) * params.max_steering)[ok].max())
        d_thr = max(d_thr, np.abs(r["cmd"][1] - h[D.REC_CMD + 1])[ok].max())
        assert np.abs(r["cte_epsi"] - h[D.REC_CTE:D.REC_EPSI + 1])[:, ok].max() <= 1e-9
        nxt = dev["hist"][t + 1, :6] if t < steps - 1 else dev["car"]
        pc = base.copy()
        pc[2] = base[2] + nz[NH.STEER] * z[t, NH.Z_STEER]; pc[5] = base[5] + nz[NH.DRIFT] * z[t, NH.Z_DRIFT]
        cmd = np.where(dropped[t], np.nan, h[D.REC_CMD:D.REC_CMD + 2])
        ref, usable = D.twin_plant_call(dt, params, h[:6], cmd, opts, plant=pc)
        assert usable.all() and (np.abs(nxt - ref) <= 4 * subs * np.spacing(np.maximum(1.0, np.abs(ref)))).all(), t
        keep = dropped[t]
        assert np.array_equal(nxt[4:6, keep], h[4:6, keep])
        assert np.array_equal(nxt[4, ~keep], h[D.REC_CMD, ~keep] * params.max_steering) and np.array_equal(nxt[5, ~keep], h[D.REC_CMD + 1, ~keep])
    print("device vs CPU build, warm %d: max |d steer| %.3g rad, |d throttle| %.3g; statuses %s; %d of %d messages dropped" % (
        warm, d_steer, d_thr, np.bincount(dev["hist"][:, D.REC_STATUS].astype(np.int64).ravel()), dropped.sum(), dropped.size))
    assert d_steer <= TOL_STEER and d_thr <= D.TOL_THROTTLE
    D.check_summary(dev, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("wave_max_batch,fused", [(0, False), (-1, False), (-1, True)])
def test_unusable_columns(pkg, golden_dir, waypoints, wave_max_batch, fused):
    """noise_helpers.UNUSABLE -- each row not-a-number and infinite, sigma = -1, p_drop = 1.5 and -0.1, seed 0.5, -1 and 2^53 -- in 24
    of 65 cars among clean ones, the rule of include/mpc_amd_noise.h, cold and warm; the drives run in a child process under a time
    limit of its own (noise_helpers.run_in_child, the arrangement of drive_helpers.run_in_child)."""
    res = NH.run_in_child(fused, wave_max_batch)
    params = _params(pkg, golden_dir, wave_max_batch=wave_max_batch)
    bad = NH.child_cases(pkg, params, waypoints)[3]
    for warm in (0, 1):
        assert res[warm, "got"]["info"] == (ONE_LAUNCH if fused else STEPWISE)
        NH.check_unusable(res[warm, "got"], res[warm, "ref"], res[warm, "zero"], bad)
        assert (res[warm, "zero"]["hist"][:, 10][:, bad] == NH.SUCCESS).mean() > 0.8
    assert not np.array_equal(res[0, "got"]["hist"][1:, D.REC_ITERS][:, bad], res[1, "got"]["hist"][1:, D.REC_ITERS][:, bad])      # (warm is not cold)


def test_host_form_and_python_layer(pkg, golden_dir, waypoints, cars200, torch_dev):
    """_host_noise is bitwise the device form at B = 7; drive_torch(noise=..., seen=True) and drive_numpy give the same results, with
    and without the other arrays; shape and dtype errors raise ValueError."""
    import torch
    params = _params(pkg, golden_dir)
    car, weights, model, lat, plant, hz, budget, nz = (a[..., :7] for a in cars200)
    nz = np.ascontiguousarray(nz)
    tx, ty = D.track_of(waypoints)
    every = dict(model=model, horizon=hz, budget=budget, latency=lat, plant=plant)
    for warm in (0, 1):
        alone = _drive(pkg, params, waypoints, car, 3, torch_dev, noise=nz, warm=warm)
        _same(alone, _drive(pkg, params, waypoints, car, 3, torch_dev, noise=nz, warm=warm, form="host"))
        full = _drive(pkg, params, waypoints, car, 3, torch_dev, noise=nz, warm=warm, weights=weights, **every)
        _same(full, _drive(pkg, params, waypoints, car, 3, torch_dev, noise=nz, warm=warm, weights=weights, form="host", **every))
        _same(full, _drive(pkg, params, waypoints, car, 3, torch_dev, noise=nz, warm=warm, weights=weights, form="host", seen=False, hist=False, **every))
        with pkg.BatchedMPC(params, 7, device=0) as mpc:
            o = mpc.drive_opts(warm_start=warm)
            for fused in (False, True):
                r = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, opts=o, fused=fused, noise=_t(nz, torch_dev), seen=True)
                torch.cuda.synchronize()
                for k in NH.KEYS:
                    assert np.array_equal(r[k].cpu().numpy(), alone[k]), (k, fused)
                r = mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, weights=_t(weights, torch_dev), opts=o, fused=fused,
                                    model=_t(model, torch_dev), latency=_t(lat, torch_dev), plant=_t(plant, torch_dev), horizon=_t(hz, torch_dev, np.int32),
                                    budget=_t(budget, torch_dev, np.int32), noise=_t(nz, torch_dev))
                torch.cuda.synchronize()
                assert r["seen"] is None and all(np.array_equal(r[k].cpu().numpy(), full[k]) for k in NH.KEYS if k != "seen"), fused
            _same(mpc.drive_numpy(car, tx, ty, 3, opts=o, noise=nz, seen=True), alone)
            _same(mpc.drive_numpy(car, tx, ty, 3, weights=weights, opts=o, noise=nz, seen=True, **every), full)
            quiet = mpc.drive_numpy(car, tx, ty, 3, opts=o)
            told = mpc.drive_numpy(car, tx, ty, 3, opts=o, seen=True)
            _same(told, quiet)
            assert quiet["seen"] is None and np.array_equal(told["seen"], told["hist"][:, 0:4])
            _same(mpc.drive_numpy(car, tx, ty, 3, opts=o, noise=mpc.drive_noise_default(7, nz[0])), quiet)
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, noise=_t(nz[:, :6], torch_dev))
            with pytest.raises(ValueError):
                mpc.drive_torch(_t(car, torch_dev), _t(tx, torch_dev), _t(ty, torch_dev), 3, noise=_t(nz, torch_dev).float())
            with pytest.raises(ValueError):
                mpc.drive_numpy(car, tx, ty, 3, noise=nz[:6])


def test_refusals_on_a_live_handle(pkg, golden_dir, waypoints, torch_dev):
    """With noise or seen an F32 handle is refused first (MPC_ERR_INVALID, the fp64-handles-only text of the drive), before what the
    _budget forms refuse: ld < B: MPC_ERR_INVALID; warm_start with max_soc > 0: MPC_ERR_UNSUPPORTED.  A refused call touches nothing
    (device_noise_drive checks every output and the cars)."""
    B = 8
    params = _params(pkg, golden_dir)
    car = pkg.scenarios.track_starts(B, params, waypoints)
    nz = NH.noise_columns(B)
    hz = mixed_horizons(B)
    for form in ("device", "fused", "host"):
        with pkg.BatchedMPC(_params(pkg, golden_dir, precision=pkg.PRECISION_F32), B, device=0) as mpc:
            for kw in (dict(noise=nz, seen=False), dict(noise=None, seen=True), dict(noise=nz, seen=True, horizon=hz)):
                text = _drive(pkg, params, waypoints, car, 2, torch_dev, form=form, mpc=mpc, expect=-1, **kw)
                assert "track driving: fp64 handles only" in text, (form, text)
            assert mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            assert "ld" in _drive(pkg, params, waypoints, car, 2, torch_dev, noise=nz, form=form, mpc=mpc, pad=-1, expect=-1)
            assert mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
        with pkg.BatchedMPC(_params(pkg, golden_dir, max_soc=4), B, device=0) as mpc:
            assert "second-order" in _drive(pkg, params, waypoints, car, 2, torch_dev, noise=nz, form=form, mpc=mpc, warm=1, expect=-4)
            assert mpc.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
            r = _drive(pkg, params, waypoints, car, 2, torch_dev, noise=nz, form=form, mpc=mpc)          # cold with SOC: served, by the stepwise loop
            assert r["info"] == STEPWISE
