"""The per-instance iteration budget on the device (mpc_solve_batch_{device,host}_budget and mpc_drive_batch_{device,device_fused,
host}_budget; include/mpc_amd_budget.h): the per-lane-rows builds of the lane kernel against handles created with max_iter = b, a
budget that does not bind, budget == NULL against the forms the entry points extend, the invariants, the warm rules, unusable values
and refusals, the three drive forms against each other and against the CPU build, and the point of the feature.  The populations
and most of the checks are those of tests/test_budget.py (tests/budget_helpers.py)."""
import ctypes as C

import numpy as np
import pytest

import budget_helpers as BH
import drive_helpers as D
import drive_latency_helpers as DL
import drive_plant_helpers as DP
from budget_helpers import INFEASIBLE, MAXITER, SUCCESS, device_budget_drive, device_budget_solve, same_columns, with_params
from drive_horizon_helpers import mixed_horizons
from helpers import TOL_STEER
from model_helpers import draw_rows

pytestmark = pytest.mark.gpu

ONE_LAUNCH, STEPWISE = {"fused_launches": 1, "stepwise_loops": 0}, {"fused_launches": 0, "stepwise_loops": 1}


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pop(pkg, golden_dir, waypoints):
    return BH.solve_population(pkg, golden_dir, waypoints)


@pytest.fixture(scope="module")
def mpc(pkg, pop):
    with pkg.BatchedMPC(pop[0], 2048, device=0) as m:
        yield m


@pytest.fixture(scope="module")
def solve(pkg, mpc, dev, pop):
    """solve(budget, **kw): the stated population through mpc_solve_batch_device_budget with the default warm options"""
    opts = pkg.warm_opts_default()
    return lambda budget, **kw: device_budget_solve(pkg, mpc, dev, pop[1], budget, opts=opts, **kw)


@pytest.fixture(scope="module")
def free(solve):
    """the population without a budget, cold, with its records: computed once, never changed"""
    return solve(None, want_warm=True)


def test_columns_are_those_of_handles_with_that_max_iter(pkg, mpc, dev, pop, solve):
    """For every budget value b the columns with that value are, bitwise, the same instances through mpc_solve_batch_device_warm_horizon
    (cold, every horizon the handle's N: the same build of the lane kernel) on a handle created with max_iter = b: out, traj, warm_out,
    status, iters, over the instances whose iters in that run is at most b; at least 90 % of every group.  The host form, ld > B and
    B = 1 write the same bits."""
    params, b, budget = pop
    B = budget.shape[0]
    opts = pkg.warm_opts_default()
    got = solve(budget, want_warm=True)
    BH.check_invariants(got, budget)
    same_columns(got, solve(budget, want_warm=True, pad=5), what="ld > B")
    same_columns(got, solve(budget, want_warm=True, pad=3, form="host"), what="host form")
    for bb in BH.BUDGETS:
        idx = np.nonzero(budget == bb)[0]
        with pkg.BatchedMPC(with_params(params, max_iter=int(bb)), 256, device=0) as m:
            yard = device_budget_solve(pkg, m, dev, b, None, horizon=np.full(B, params.N, dtype=np.int32), opts=opts, want_warm=True, entry="warm_horizon")
        cmp = idx[yard["iters"][idx] <= bb]
        assert len(idx) > 0 and len(cmp) >= 0.9 * len(idx), (bb, len(idx), len(cmp))
        same_columns(got, yard, cmp, what="budget %d" % bb)
    for i in (0, 192):
        one = device_budget_solve(pkg, mpc, dev, BH.sub_batch(b, [i]), budget[[i]], opts=opts, want_warm=True, pad=2)
        same_columns(one, {k: v[..., [i]] for k, v in got.items()}, what="B = 1, instance %d" % i)


def test_a_budget_that_does_not_bind_changes_nothing(pkg, mpc, dev, pop, solve, free, waypoints):
    """budget[i] at the instance's unbudgeted iters and above: bitwise budget == NULL, cold and warm.  budget == NULL is bitwise
    mpc_solve_batch_device_warm_horizon / _host_warm_horizon at B = 1, 193 and 1 100 (above wave_max_batch = 1 024), with horizons and
    with horizon == NULL -- where the form is the wave kernel's up to the limit and the staged lane kernel's above."""
    params, b, _ = pop
    opts = pkg.warm_opts_default()
    assert (free["status"] != MAXITER).all()
    warm_free = solve(None, warm=free["warm"], warm_status=free["status"])
    assert warm_free["iters"].mean() < 0.6 * free["iters"].mean()
    for extra in (0, 50):
        same_columns(solve(free["iters"] + extra, want_warm=True), free, what="cold +%d" % extra)
        same_columns(solve(np.maximum(warm_free["iters"], 1) + extra, warm=free["warm"], warm_status=free["status"]), warm_free, what="warm +%d" % extra)
    big = pkg.scenarios.lake_track_batch(1100, params, waypoints, seed=5)
    big = {k: np.ascontiguousarray(big[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    assert params.wave_max_batch in (0, 1024)
    for batch in (BH.sub_batch(b, [5]), b, big):
        n = batch["state"].shape[1]
        hz = np.random.default_rng(3).choice([3, 5, 10], n).astype(np.int32)
        for h in (None, hz):
            for form in ("device", "host"):
                a = device_budget_solve(pkg, mpc, dev, batch, None, horizon=h, opts=opts, want_warm=True, form=form, pad=1)
                ref = device_budget_solve(pkg, mpc, dev, batch, None, horizon=h, opts=opts, want_warm=True, form=form, pad=1, entry="warm_horizon")
                same_columns(a, ref, what="budget NULL, B = %d" % n)
                w = device_budget_solve(pkg, mpc, dev, batch, None, horizon=h, opts=opts, warm=a["warm"], warm_status=a["status"], form=form)
                same_columns(w, device_budget_solve(pkg, mpc, dev, batch, None, horizon=h, opts=opts, warm=a["warm"], warm_status=a["status"], form=form,
                                                    entry="warm_horizon"), what="budget NULL, warm, B = %d" % n)


def test_invariants_warm_and_with_the_other_columns(pkg, mpc, dev, pop, solve, free):
    """iters <= b, MAXITER exactly at iters == b without a convergence test, nothing not-a-number: warm from the records of a budgeted
    call, and with model, horizon and weights in the call; where the unbudgeted solve needs at most b the instance is that solve."""
    params, b, budget = pop
    B = budget.shape[0]
    opts = pkg.warm_opts_default()
    cold = solve(budget, want_warm=True)
    binds = free["iters"] > budget
    assert (cold["iters"][binds] == budget[binds]).all() and np.isin(cold["status"][binds], (MAXITER, SUCCESS)).all()
    same_columns(cold, free, np.nonzero(~binds)[0], what="not binding")
    BH.check_invariants(solve(budget, warm=cold["warm"], warm_status=cold["status"]), budget, "warm")
    model, hz = draw_rows(params, B), np.random.default_rng(3).choice([3, 5, 10], B).astype(np.int32)
    weights = pkg.scenarios.weight_sweep(B, params, seed=91)
    unb = device_budget_solve(pkg, mpc, dev, b, None, horizon=hz, model=model, weights=weights, opts=opts, want_warm=True)
    got = device_budget_solve(pkg, mpc, dev, b, budget, horizon=hz, model=model, weights=weights, opts=opts, want_warm=True)
    ok = unb["status"] != INFEASIBLE
    assert ok.sum() > 150 and (got["status"][~ok] == INFEASIBLE).all()
    st, it = got["status"][ok], got["iters"][ok]
    assert (it <= budget[ok]).all() and ((st == MAXITER) <= (it == budget[ok])).all() and np.isfinite(got["out"]).all()
    same_columns(got, unb, np.nonzero(ok & (unb["iters"] <= budget))[0], keys=("out", "status", "iters"), what="not binding, with columns")


def test_warm_rules(pop, solve, free):
    """tests/test_budget.py::test_warm_rules on the device."""
    assert BH.check_warm_rules(solve, free, pop[0].N) >= 20


def test_unusable_budgets(pop, solve):
    """tests/test_budget.py::test_unusable_budgets on the device."""
    BH.check_unusable(solve, pop[1], pop[2], pop[0].N)


def test_solve_refusals(pkg, dev, pop, golden_dir):
    """An MPC_PRECISION_F32 handle: MPC_ERR_INVALID with the model message; max_soc > 0 with a budget: MPC_ERR_UNSUPPORTED, naming both;
    budget == NULL on that handle: the extended form's own refusal (a warm call with SOC); ld_warm < B as ever.  A refused call writes
    nothing."""
    params, b, budget = pop
    opts = pkg.warm_opts_default()
    sb = BH.sub_batch(b, list(range(8)))
    with pkg.BatchedMPC(with_params(params, precision=pkg.PRECISION_F32), 8, device=0) as m:
        for form in ("device", "host"):
            assert "per-instance model values: fp64 handles only" in device_budget_solve(pkg, m, dev, sb, budget[:8], opts=opts, form=form, expect=-1)
    with pkg.BatchedMPC(with_params(params, max_soc=4), 8, device=0) as m:
        for form in ("device", "host"):
            msg = device_budget_solve(pkg, m, dev, sb, budget[:8], opts=opts, form=form, expect=-4)
            assert "budget" in msg and "second-order correction" in msg
            msg = device_budget_solve(pkg, m, dev, sb, None, opts=opts, form=form, want_warm=True, expect=-4)
            assert "warm start is not available with the second-order correction" in msg


# ---- the drive ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dpop(pkg, golden_dir, waypoints):
    return BH.drive_population(pkg, golden_dir, waypoints)


@pytest.fixture(scope="module")
def drives(pkg, dev, dpop, waypoints):
    """the stated drive in one launch, cold and warm: without a budget and with the stated budgets; computed once, never changed"""
    params, car, budget = dpop
    res = {}
    for warm in (0, 1):
        res[warm, "free"] = device_budget_drive(pkg, params, waypoints, car, BH.DRIVE_STEPS, dev, None, form="fused", warm=warm)
        res[warm, "budget"] = device_budget_drive(pkg, params, waypoints, car, BH.DRIVE_STEPS, dev, budget, form="fused", warm=warm)
    return res


@pytest.mark.parametrize("warm", [0, 1])
def test_drive_forms_write_the_same_bits(pkg, dev, dpop, drives, waypoints, warm):
    """Stepwise, fused and host forms with the stated budgets: bitwise the same, at B = 70, B = 1 and with hist == NULL; mpc_drive_info
    counts the one launch where _fused_horizon's rule says it runs -- at every B, below the wave limit too -- and the stepwise loop
    elsewhere.  Invariants on every step; summary rows from the records."""
    params, car, budget = dpop
    r = drives[warm, "budget"]
    assert r["info"] == ONE_LAUNCH
    BH.check_drive_invariants(r, budget)
    D.check_summary(r, len(waypoints), pkg.drive_opts_default(params).cte_limit)
    assert (r["hist"][:, D.REC_STATUS] == MAXITER).sum() > 100
    step = device_budget_drive(pkg, params, waypoints, car, BH.DRIVE_STEPS, dev, budget, form="device", warm=warm)
    host = device_budget_drive(pkg, params, waypoints, car, BH.DRIVE_STEPS, dev, budget, form="host", warm=warm)
    assert step["info"] == STEPWISE and host["info"] == STEPWISE
    D.same(step, r); D.same(host, r)
    D.same(device_budget_drive(pkg, params, waypoints, car, BH.DRIVE_STEPS, dev, budget, form="fused", warm=warm, hist=False), r)
    for i in (0, 69):
        for form, info in (("fused", ONE_LAUNCH), ("device", STEPWISE)):
            one = device_budget_drive(pkg, params, waypoints, car[:, i:i + 1], BH.DRIVE_STEPS, dev, budget[i:i + 1], form=form, warm=warm)
            assert one["info"] == info
            D.same(one, {k: r[k][..., i:i + 1] for k in D.KEYS})


@pytest.mark.parametrize("warm", [0, 1])
def test_drive_null_and_a_budget_that_does_not_bind(pkg, dev, dpop, drives, waypoints, warm):
    """budget == NULL is bitwise the _plant form, with its dispatch and info counters: the three forms, plain (the wave kernels below the
    limit) and with model, horizon, latency and plant.  A budget at or above every step's unbudgeted iterations is bitwise budget ==
    NULL; the budget-50 cars of the stated batch are bitwise their unbudgeted selves."""
    params, car, budget = dpop
    B = car.shape[1]
    model, lat, plant, hz = draw_rows(params, B, seed=9), DL.draw_latency(B), DP.draw_plant(B), mixed_horizons(B)
    for form in ("device", "fused", "host"):
        for kw in ({}, {"model": model, "horizon": hz, "latency": lat, "plant": plant}):
            a = device_budget_drive(pkg, params, waypoints, car, 4, dev, None, form=form, warm=warm, **kw)
            ref = D.device_drive(pkg, params, waypoints, car, 4, dev, form=form, warm=warm, **kw)
            D.same(a, ref)
            assert a["info"] == ref["info"], (form, bool(kw))
    f, r = drives[warm, "free"], drives[warm, "budget"]
    assert (f["hist"][:, D.REC_STATUS] != MAXITER).all()
    top = int(f["hist"][:, D.REC_ITERS].max())
    D.same(device_budget_drive(pkg, params, waypoints, car, BH.DRIVE_STEPS, dev, np.full(B, top, dtype=np.int32), form="fused", warm=warm), f)
    D.same(r, f, cars=np.nonzero((budget == 50) & (f["hist"][:, D.REC_ITERS].max(0) <= 50))[0])


@pytest.mark.parametrize("warm", [0, 1])
def test_drive_columns_combine(pkg, dev, dpop, waypoints, warm):
    """model, horizon, latency, plant and weights with budget in one mixed batch: fused bitwise stepwise; a budget that does not bind is
    bitwise the _plant form with the same columns; the invariants hold under the stated budgets."""
    params, car, budget = dpop
    B = car.shape[1]
    kw = {"model": draw_rows(params, B, seed=9), "latency": DL.draw_latency(B), "plant": DP.draw_plant(B), "horizon": mixed_horizons(B),
          "weights": pkg.scenarios.weight_sweep(B, params, seed=91)}
    ref = D.device_drive(pkg, params, waypoints, car, 6, dev, form="fused", warm=warm, **kw)
    assert (ref["hist"][:, D.REC_STATUS] != MAXITER).all()
    D.same(device_budget_drive(pkg, params, waypoints, car, 6, dev, np.full(B, 1000, dtype=np.int32), form="fused", warm=warm, **kw), ref)
    a = device_budget_drive(pkg, params, waypoints, car, 6, dev, budget, form="fused", warm=warm, **kw)
    b = device_budget_drive(pkg, params, waypoints, car, 6, dev, budget, form="device", warm=warm, **kw)
    assert a["info"] == ONE_LAUNCH and b["info"] == STEPWISE
    D.same(a, b)
    BH.check_drive_invariants(a, budget)


@pytest.mark.parametrize("warm", [0, 1])
def test_drive_against_the_cpu_build(pkg, dev, dpop, drives, waypoints, warm):
    """The stated drive against tests/drive_twin/budget_drive_twin.cpp as tests/test_drive_plant_gpu.py::test_stepwise_against_the_cpu_build
    compares: windows and statuses equal at every step, and the iterations of every step the budget ended; the replies compared solve by solve -- the CPU build's handler
    re-run on the device's recorded car and window, its own records handed from step to step -- within TOL_STEER and TOL_THROTTLE,
    cte and epsi within 1e-9."""
    params, car, budget = dpop
    twin = BH.load_budget_drive_twin()
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    dv = drives[warm, "budget"]
    tw = BH.twin_budget_drive(twin, params, waypoints, car, BH.DRIVE_STEPS, opts, wopts, budget)
    on_road = np.nonzero(tw["summary"][6] < 0)[0]
    assert np.array_equal(dv["hist"][:, D.REC_K][:, on_road], tw["hist"][:, D.REC_K][:, on_road])
    mem = {"warm": None, "status": None}
    d_steer = d_thr = 0.0
    for t in range(BH.DRIVE_STEPS):
        h = dv["hist"][t]
        r = BH.twin_budget_handler(twin, params, waypoints, h[:6], h[D.REC_K].astype(np.int32), opts, wopts, budget, warm=mem["warm"] if warm else None,
                                   warm_status=mem["status"] if warm else None, want_warm=bool(warm))
        mem["warm"], mem["status"] = r["warm"], r["status"]
        assert np.array_equal(r["status"], h[D.REC_STATUS].astype(np.int32)), t
        ok = np.isin(r["status"], (SUCCESS, MAXITER))
        cut = r["status"] == MAXITER
        assert np.array_equal(r["iters"][cut], h[D.REC_ITERS].astype(np.int32)[cut]) and (r["iters"][cut] == budget[cut]).all(), t
        d_steer = max(d_steer, (np.abs(r["cmd"][0] - h[D.REC_CMD]) * params.max_steering)[ok].max())
        d_thr = max(d_thr, np.abs(r["cmd"][1] - h[D.REC_CMD + 1])[ok].max())
        assert np.abs(r["cte_epsi"] - h[D.REC_CTE:D.REC_EPSI + 1])[:, ok].max() <= 1e-9
    print("device vs CPU build, warm %d: max |d steer| %.3g rad, |d throttle| %.3g; statuses %s" % (
        warm, d_steer, d_thr, np.bincount(dv["hist"][:, D.REC_STATUS].astype(np.int64).ravel())))
    assert d_steer <= TOL_STEER and d_thr <= D.TOL_THROTTLE


def test_drive_unusable_budgets_and_refusals(pkg, dev, dpop, drives, waypoints):
    """A car with budget 0, -1 or INT32_MIN ends every step INFEASIBLE with finite rows, every other car is bitwise the batch without the
    defect (one launch and stepwise).  An MPC_PRECISION_F32 handle is refused with the drive's fp64-handles text (the extended form's
    first refusal), max_soc > 0 with a budget with MPC_ERR_UNSUPPORTED naming both; a refused call touches nothing."""
    import torch
    params, car, budget = dpop
    B = car.shape[1]
    bad = np.array([2, 63, 64, 69])
    dirty = budget.copy(); dirty[bad] = [0, -1, BH.INT32_MIN, 0]
    good = np.setdiff1d(np.arange(B), bad)
    for warm in (0, 1):
        for form in ("fused", "device"):
            got = device_budget_drive(pkg, params, waypoints, car, BH.DRIVE_STEPS, dev, dirty, form=form, warm=warm)
            D.same(got, drives[warm, "budget"], cars=good)
            assert (got["hist"][:, D.REC_STATUS][:, bad] == INFEASIBLE).all() and (got["status"][bad] == INFEASIBLE).all() and (got["iters"][bad] == 0).all()
            assert (got["summary"][7, bad] == BH.DRIVE_STEPS).all()
            for k in ("car", "summary", "hist"):
                assert np.isfinite(got[k]).all(), k
    lib = pkg.library()
    tx, ty = D.track_of(waypoints)
    t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_car, d_bg, d_tx, d_ty = t(car), t(budget, np.int32), t(tx), t(ty)
    summ = torch.full((8, B), D.SENTINEL, dtype=torch.float64, device=dev); st = torch.full((B,), D.ISENTINEL, dtype=torch.int32, device=dev)
    before = d_car.clone()
    good_opts = pkg.drive_opts_default(params)

    def call(h, name):
        return getattr(lib, name)(h, B, B, 2, d_car.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(), len(tx), None, None, None, d_bg.data_ptr(), None, None,
                                  C.byref(good_opts), None, summ.data_ptr(), None, st.data_ptr(), None, None)
    names = ("mpc_drive_batch_device_budget", "mpc_drive_batch_device_fused_budget")
    with pkg.BatchedMPC(with_params(params, precision=pkg.PRECISION_F32), B, device=0) as m:
        for name in names:
            assert call(m._h, name) == -1 and b"fp64 handles only" in lib.mpc_last_error()
    with pkg.BatchedMPC(with_params(params, max_soc=4), B, device=0) as m:
        for name in names:
            assert call(m._h, name) == -4 and b"budget" in lib.mpc_last_error() and b"second-order correction" in lib.mpc_last_error()
        assert m.drive_info() == {"fused_launches": 0, "stepwise_loops": 0}
    torch.cuda.synchronize()
    assert torch.equal(d_car, before) and bool((summ == D.SENTINEL).all()) and bool((st == D.ISENTINEL).all())


def test_python_layer(pkg, dev, dpop, drives, pop, solve, waypoints):
    """solve_torch(budget=), solve_numpy_warm(budget=), drive_torch(budget=) and drive_numpy(budget=) give the raw calls' results; shape
    and dtype errors raise ValueError."""
    import torch
    params, b, budget = pop
    t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    raw = solve(budget, want_warm=True)
    with pkg.BatchedMPC(params, 256, device=0) as m:
        r = m.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), want_traj=True, want_warm=True, budget=t(budget, np.int32))
        torch.cuda.synchronize()
        same_columns({k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}, raw)
        r = m.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), budget=t(budget, np.int32))
        torch.cuda.synchronize()
        same_columns({k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}, raw, keys=("out", "status", "iters"))
        same_columns(m.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], want_traj=True, budget=budget), raw)
        with pytest.raises(ValueError):
            m.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), budget=t(budget[:-1], np.int32))
        with pytest.raises(ValueError):
            m.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), budget=t(budget, np.int64))
    params, car, budget = dpop
    tx, ty = D.track_of(waypoints)
    with pkg.BatchedMPC(params, 128, device=0) as m:
        for warm in (0, 1):
            o = m.drive_opts(warm_start=warm)
            ref = drives[warm, "budget"]
            for fused in (False, True):
                r = m.drive_torch(t(car), t(tx), t(ty), BH.DRIVE_STEPS, opts=o, fused=fused, budget=t(budget, np.int32))
                torch.cuda.synchronize()
                D.same({k: r[k].cpu().numpy() for k in D.KEYS}, ref)
            D.same(m.drive_numpy(car, tx, ty, BH.DRIVE_STEPS, opts=o, budget=budget), ref)
        with pytest.raises(ValueError):
            m.drive_torch(t(car), t(tx), t(ty), 2, budget=t(budget[:-1], np.int32))
        with pytest.raises(ValueError):
            m.drive_numpy(car, tx, ty, 2, budget=budget.astype(np.int64))


def test_warm_start_is_what_a_small_budget_needs(dpop, drives):
    """tests/test_budget.py::test_warm_start_is_what_a_small_budget_needs on the device's drives: the same cars and budgets, cold and warm
    (two calls: warm_start is an option of the call), the same ordering on the b = 2 group."""
    BH.check_the_point(drives[0, "budget"], drives[1, "budget"], drives[0, "free"], dpop[2], tag="device: ")
