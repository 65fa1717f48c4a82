"""The per-instance iteration budget on the CPU builds (tests/host_twin/budget_twin.cpp, tests/drive_twin/budget_drive_twin.cpp; the
rules are mpc::Solver's "iteration budget" in csrc/mpc_core.h, which the kernels share): the budget against handles created with
max_iter = b, a budget that does not bind, the invariants, the warm rules, unusable values, the drive, and the point of the feature --
warm-started cars under a small budget.  Populations: budget_helpers.solve_population (config-fast.json at N = 10, B = 193, budgets
from {1, 2, 3, 5, 8, 13, 200}) and drive_population (70 cars x 12 messages on the lake track, budgets from {2, 4, 8, 50})."""
import numpy as np
import pytest

import budget_helpers as BH
import drive_helpers as D
import drive_latency_helpers as DL
import drive_plant_helpers as DP
import horizon_helpers as HH
from budget_helpers import INFEASIBLE, MAXITER, SUCCESS, same_columns, twin_budget_drive, twin_budget_solve, with_params
from drive_horizon_helpers import mixed_horizons
from model_helpers import draw_rows


@pytest.fixture(scope="module")
def twin():
    return BH.load_budget_twin()


@pytest.fixture(scope="module")
def drive_twin():
    return BH.load_budget_drive_twin()


@pytest.fixture(scope="module")
def pop(pkg, golden_dir, waypoints):
    return BH.solve_population(pkg, golden_dir, waypoints)


@pytest.fixture(scope="module")
def free(pkg, twin, pop):
    """the population without a budget, cold, with its records: computed once, never changed"""
    params, b, _ = pop
    return twin_budget_solve(twin, params, b, None, want_warm=True, opts=pkg.warm_opts_default())


def _full_N(params, B):
    return np.full(B, params.N, dtype=np.int32)


def test_columns_are_those_of_handles_with_that_max_iter(pkg, twin, pop):
    """For every budget value b the columns with that value are, bitwise, the same instances through the _warm_horizon form (cold; its
    CPU build, tests/host_twin/horizon_twin.cpp) with max_iter = b: out, traj, warm_out, status, iters -- over the instances whose
    iters in that yardstick run is at most b (no restart added iterations there, and the two rules coincide).  At least 90 % of every
    column group is compared (this population: all of it).  Once more at ld > B, and each instance alone at B = 1."""
    params, b, budget = pop
    B = budget.shape[0]
    opts = pkg.warm_opts_default()
    ht = HH.load_horizon_twin()
    got = twin_budget_solve(twin, params, b, budget, want_warm=True, opts=opts)
    wide = twin_budget_solve(twin, params, b, budget, want_warm=True, opts=opts, pad=5)
    same_columns(got, wide, what="ld > B")
    for bb in BH.BUDGETS:
        idx = np.nonzero(budget == bb)[0]
        yard = HH.twin_horizon_solve(ht, with_params(params, max_iter=int(bb)), b, _full_N(params, B), opts, want_warm=True)
        cmp = idx[yard["iters"][idx] <= bb]
        assert len(idx) > 0 and len(cmp) >= 0.9 * len(idx), (bb, len(idx), len(cmp))
        same_columns(got, yard, cmp, what="budget %d" % bb)
    for i in (0, 7, 100, 192):
        one = twin_budget_solve(twin, params, BH.sub_batch(b, [i]), budget[[i]], want_warm=True, opts=opts, pad=2)
        same_columns(one, {k: v[..., [i]] for k, v in got.items()}, what="B = 1, instance %d" % i)


def test_invariants(pkg, twin, pop, free):
    """iters <= b everywhere; MAXITER exactly where iters == b and neither convergence test held; no not-a-number -- cold, and warm from
    the records of a budgeted call (MAXITER records among them)."""
    params, b, budget = pop
    opts = pkg.warm_opts_default()
    cold = twin_budget_solve(twin, params, b, budget, want_warm=True, opts=opts)
    BH.check_invariants(cold, budget, "cold")
    assert (cold["status"] == MAXITER).sum() > 100 and (cold["status"] == SUCCESS).sum() > 20
    # (where the unbudgeted solve needs more than b, the budget ends it at b -- MAXITER, or SUCCESS where the convergence test holds at
    # iteration b and only the polish would have gone on --; where it needs at most b, it is that solve)
    binds = free["iters"] > budget
    assert (cold["iters"][binds] == budget[binds]).all() and np.isin(cold["status"][binds], (MAXITER, SUCCESS)).all()
    assert (cold["status"][binds] == MAXITER).mean() > 0.95
    same_columns(cold, free, np.nonzero(~binds)[0], what="not binding")
    warm = twin_budget_solve(twin, params, b, budget, warm=cold["warm"], warm_status=cold["status"], opts=opts)
    BH.check_invariants(warm, budget, "warm")


def test_a_budget_that_does_not_bind_changes_nothing(pkg, twin, pop, free):
    """budget[i] equal to the instance's unbudgeted iters, and above it: every output is bitwise that of budget == NULL -- cold, and warm
    from the cold records (none of which came with MAXITER, so the wider warm rule admits no other record).  budget == NULL is bitwise
    the _warm_horizon form's CPU build at B = 1 and B = 193, with and without horizons."""
    params, b, _ = pop
    B = free["iters"].shape[0]
    opts = pkg.warm_opts_default()
    assert (free["status"] != MAXITER).all()
    for shift in (0, 1):
        wo = pkg.warm_opts_default(shift=shift)
        warm_free = twin_budget_solve(twin, params, b, None, warm=free["warm"], warm_status=free["status"], opts=wo)
        assert warm_free["iters"].mean() < 0.6 * free["iters"].mean()
        for extra in (0, 1, 50):
            same_columns(twin_budget_solve(twin, params, b, free["iters"] + extra, want_warm=True, opts=opts), free, what="cold +%d" % extra)
            got = twin_budget_solve(twin, params, b, np.maximum(warm_free["iters"], 1) + extra, warm=free["warm"], warm_status=free["status"], opts=wo)
            same_columns(got, warm_free, what="warm +%d" % extra)
    ht = HH.load_horizon_twin()
    hz = HH.draw_horizons(B, choices=HH.LOOP_HORIZONS)
    for idx in ([5], list(range(B))):
        sb = BH.sub_batch(b, idx)
        for h in (None, hz[idx]):
            a = twin_budget_solve(twin, params, sb, None, horizon=h, want_warm=True, opts=opts)
            ref = HH.twin_horizon_solve(ht, params, sb, h if h is not None else _full_N(params, len(idx)), opts, want_warm=True)
            same_columns(a, ref, what="budget NULL, B = %d" % len(idx))


def test_warm_rules(pkg, twin, pop, free):
    """A MAXITER record is taken warm with a budget and refused without one; a warm attempt that ends by budget is final; a refused
    record starts cold under the same total; a warm attempt that fails otherwise is followed by a cold solve with the remainder -- one
    is constructed from the converged records with x and y moved by 50 m (budget_helpers.far_records): 69 instances of this
    population fail their warm attempt after 1 .. 4 iterations."""
    params, b, _ = pop
    opts = pkg.warm_opts_default()
    n = BH.check_warm_rules(lambda budget, **kw: twin_budget_solve(twin, params, b, budget, opts=opts, **kw), free, params.N)
    assert n >= 20


def test_unusable_budgets(pkg, twin, pop):
    """0, -1 and INT32_MIN: MPC_STATUS_INFEASIBLE with the start point, no not-a-number, iters 0; every other instance is bitwise what it
    is without the defect -- cold and warm."""
    params, b, budget = pop
    opts = pkg.warm_opts_default()
    BH.check_unusable(lambda budget, **kw: twin_budget_solve(twin, params, b, budget, opts=opts, **kw), b, budget, params.N)


# ---- the drive ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dpop(pkg, golden_dir, waypoints):
    return BH.drive_population(pkg, golden_dir, waypoints)


@pytest.fixture(scope="module")
def drives(pkg, drive_twin, dpop, waypoints):
    """the stated drive, cold and warm: without a budget and with the stated budgets; computed once, never changed"""
    params, car, budget = dpop
    wo = pkg.warm_opts_default()
    res = {}
    for warm in (0, 1):
        o = pkg.drive_opts_default(params, warm_start=warm)
        res[warm, "free"] = twin_budget_drive(drive_twin, params, waypoints, car, BH.DRIVE_STEPS, o, wo, None)
        res[warm, "budget"] = twin_budget_drive(drive_twin, params, waypoints, car, BH.DRIVE_STEPS, o, wo, budget)
    return res


def test_drive_null_budget_is_the_plant_form(pkg, drive_twin, dpop, drives, waypoints):
    """budget == NULL is bitwise tests/drive_twin's loop (the _plant form's CPU build): plain, and with model, horizon, latency and plant;
    at B = 1 too."""
    params, car, _ = dpop
    B = car.shape[1]
    dt = D.load_drive_twin()
    wo = pkg.warm_opts_default()
    model, lat, plant, hz = draw_rows(params, B, seed=9), DL.draw_latency(B), DP.draw_plant(B), mixed_horizons(B)
    for warm in (0, 1):
        o = pkg.drive_opts_default(params, warm_start=warm)
        D.same(drives[warm, "free"], D.twin_drive_call(dt, params, waypoints, car, BH.DRIVE_STEPS, o, wo))
        a = twin_budget_drive(drive_twin, params, waypoints, car, 4, o, wo, None, model=model, horizon=hz, latency=lat, plant=plant)
        D.same(a, D.twin_drive_call(dt, params, waypoints, car, 4, o, wo, model=model, horizon=hz, latency=lat, plant=plant))
        a = twin_budget_drive(drive_twin, params, waypoints, car[:, 5:6], 4, o, wo, None)
        D.same(a, D.twin_drive_call(dt, params, waypoints, car[:, 5:6], 4, o, wo))


def test_drive_invariants_and_a_budget_that_does_not_bind(pkg, drive_twin, dpop, drives, waypoints):
    """Every step of every car: iters <= b, MAXITER exactly at iters == b without a convergence test, nothing not-a-number; summary row
    7 counts the steps that did not end SUCCESS, MAXITER steps among them.  A budget at or above every step's unbudgeted iterations is
    bitwise budget == NULL, cold and warm (no unbudgeted step ends MAXITER, so the wider warm rule admits nothing else); the budget-50
    cars of the stated batch are bitwise their unbudgeted selves.  B = 1 is its column of the batch."""
    params, car, budget = dpop
    B = car.shape[1]
    wo = pkg.warm_opts_default()
    for warm in (0, 1):
        o = pkg.drive_opts_default(params, warm_start=warm)
        r, f = drives[warm, "budget"], drives[warm, "free"]
        BH.check_drive_invariants(r, budget, "warm %d" % warm)
        D.check_summary(r, len(waypoints), o.cte_limit)
        assert np.array_equal(r["hist"][:, D.REC_STATUS].astype(np.int32), r["handler_status"])
        assert (r["hist"][:, D.REC_STATUS] == MAXITER).sum() > 100
        assert (f["hist"][:, D.REC_STATUS] != MAXITER).all()
        top = int(f["hist"][:, D.REC_ITERS].max())
        assert top <= 50
        D.same(twin_budget_drive(drive_twin, params, waypoints, car, BH.DRIVE_STEPS, o, wo, np.full(B, top, dtype=np.int32)), f)
        D.same(r, f, cars=np.nonzero(budget == 50)[0])
        for i in (0, 1, 69):
            one = twin_budget_drive(drive_twin, params, waypoints, car[:, i:i + 1], BH.DRIVE_STEPS, o, wo, budget[i:i + 1])
            D.same(one, {k: r[k][..., i:i + 1] for k in D.KEYS})


def test_drive_warm_rule(pkg, drive_twin, dpop, drives, waypoints):
    """From step 2 on, with warm_start and a budget, a car whose previous step ended SUCCESS or MAXITER starts warm: replayed handler call
    by handler call on the recorded cars and windows, a step after a MAXITER step is the handler started from that step's record, and
    differs from the handler started cold; the same records offered without a budget are refused."""
    params, car, budget = dpop
    wo = pkg.warm_opts_default()
    o = pkg.drive_opts_default(params, warm_start=1)
    r = drives[1, "budget"]
    warm, status = None, None
    seen = 0
    for t in range(6):
        h = r["hist"][t]
        k = h[D.REC_K].astype(np.int32)
        got = BH.twin_budget_handler(drive_twin, params, waypoints, h[:6], k, o, wo, budget, warm=warm, warm_status=status, want_warm=True)
        assert np.array_equal(got["status"], h[D.REC_STATUS].astype(np.int32)) and np.array_equal(got["iters"], h[D.REC_ITERS].astype(np.int32)), t
        assert np.array_equal(got["cmd"], h[D.REC_CMD:D.REC_CMD + 2]), t
        if t > 0:
            after = np.nonzero(status == MAXITER)[0]
            cold = BH.twin_budget_handler(drive_twin, params, waypoints, h[:6], k, o, wo, budget, want_warm=True)
            nobud = BH.twin_budget_handler(drive_twin, params, waypoints, h[:6], k, o, wo, None, warm=warm, warm_status=status, want_warm=True)
            free_cold = BH.twin_budget_handler(drive_twin, params, waypoints, h[:6], k, o, wo, None, want_warm=True)
            seen += int((got["cmd"][:, after] != cold["cmd"][:, after]).any(0).sum())
            assert np.array_equal(nobud["cmd"][:, after], free_cold["cmd"][:, after]) and np.array_equal(nobud["iters"][after], free_cold["iters"][after])
        warm, status = got["warm"], got["status"]
    assert seen > 50


def test_drive_columns_combine(pkg, drive_twin, dpop, waypoints):
    """model, horizon, latency and plant with budget in one mixed batch: a budget that does not bind is bitwise the _plant form's CPU
    build with the same columns; the stated budgets keep the invariants, and the cars with budget 50 are bitwise the unbudgeted ones."""
    params, car, budget = dpop
    B = car.shape[1]
    dt = D.load_drive_twin()
    wo = pkg.warm_opts_default()
    model, lat, plant, hz = draw_rows(params, B, seed=9), DL.draw_latency(B), DP.draw_plant(B), mixed_horizons(B)
    for warm in (0, 1):
        o = pkg.drive_opts_default(params, warm_start=warm)
        ref = D.twin_drive_call(dt, params, waypoints, car, 6, o, wo, model=model, horizon=hz, latency=lat, plant=plant)
        assert (ref["hist"][:, D.REC_STATUS] != MAXITER).all() and ref["hist"][:, D.REC_ITERS].max() <= 200
        D.same(twin_budget_drive(drive_twin, params, waypoints, car, 6, o, wo, np.full(B, 200, dtype=np.int32), model=model, horizon=hz, latency=lat, plant=plant), ref)
        r = twin_budget_drive(drive_twin, params, waypoints, car, 6, o, wo, budget, model=model, horizon=hz, latency=lat, plant=plant)
        BH.check_drive_invariants(r, budget)
        big = np.nonzero((budget == 50) & (ref["hist"][:, D.REC_ITERS].max(0) <= 50))[0]
        assert len(big) >= 10
        D.same(r, ref, cars=big)


def test_drive_unusable_budgets(pkg, drive_twin, dpop, drives, waypoints):
    """A car with budget 0, -1 or INT32_MIN ends every step INFEASIBLE (the rule of an unusable horizon), with finite rows; every other
    car is bitwise the batch without the defect."""
    params, car, budget = dpop
    B = car.shape[1]
    wo = pkg.warm_opts_default()
    bad = np.array([2, 63, 64, 69])
    dirty = budget.copy(); dirty[bad] = [0, -1, BH.INT32_MIN, 0]
    good = np.setdiff1d(np.arange(B), bad)
    for warm in (0, 1):
        o = pkg.drive_opts_default(params, warm_start=warm)
        got = twin_budget_drive(drive_twin, params, waypoints, car, BH.DRIVE_STEPS, o, wo, dirty)
        D.same(got, drives[warm, "budget"], cars=good)
        assert (got["hist"][:, D.REC_STATUS][:, bad] == INFEASIBLE).all() and (got["status"][bad] == INFEASIBLE).all() and (got["iters"][bad] == 0).all()
        assert (got["summary"][7, bad] == BH.DRIVE_STEPS).all()
        for k in ("car", "summary", "hist"):
            assert np.isfinite(got[k]).all(), k


def test_warm_start_is_what_a_small_budget_needs(pkg, dpop, drives):
    """The point of the feature, on the stated drive (70 cars x 12 messages, budgets {2, 4, 8, 50} in interleaved groups).  warm_start is
    an option of the call (MpcDriveOpts), so the cold and the warm cars are the same cars and budgets in two calls, not two halves of
    one.  Found on the CPU build, uniform budgets 1 .. 8 and 50 (median of summary row 0, max |cte| [m], over the 70 cars; cars that leave
    the road, row 6 >= 0): unbudgeted 0.547 / 6; cold b = 8: 0.549 / 6, b = 4: 0.557 / 6, b = 3: 0.806 / 6, b = 2: 1.556 / 9,
    b = 1: 2.124 / 21; warm b = 4: 0.538 / 6, b = 2: 0.593 / 9, b = 1: 0.693 / 15.  Of the stated budgets, b = 2 is the one at which cold
    cars measurably degrade (b = 4 is within 2 % of the unbudgeted drive, which is the largest budget that shows anything at all), so
    the ordering is asserted on the b = 2 group: warm-started, its median max |cte| is smaller than cold -- and less than half way from
    the unbudgeted value to the cold one --, more of its cars improve than get worse, and no more of them leave the road, none earlier.
    The b = 50 group is the control: its budget does not bind, and cold and warm agree to solver tolerance."""
    _, _, budget = dpop
    BH.check_the_point(drives[0, "budget"], drives[1, "budget"], drives[0, "free"], budget)
