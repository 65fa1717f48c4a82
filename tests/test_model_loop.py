"""Warm starts and closed loops with per-instance model values (include/mpc_amd.h: mpc_solve_batch_*_warm_model,
mpc_rollout_batch_device_warm_model, mpc_rollout_batch_device_fused_model), checked without a GPU: the CPU build tests/host_twin (mpc_twin_solve / mpc_twin_rollout)
calls the same Solver::setup / solve_warm / warm_store / unpack (on the instance's model column) and mpc::RolloutCar as the WARM+MODEL and ROLL+MODEL builds
of the lane kernel.  Yardsticks: the plain twins (uniform rows), the cold loop, and the oracle's own cold loop with one OrcConfig per
car."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ
from model_helpers import INFEASIBLE, population
from model_loop_helpers import (MODES, assert_loops_follow_oracle, load_model_loop_twin, oracle_model_loops, steering_outside,
                                twin_model_rollout, twin_model_step_loop, twin_warm_model_solve)
from rollout_fused_helpers import load_rollout_twin, twin_rollout
from warm_helpers import garbage_warm, load_warm_twin, twin_closed_loop

CARS, STEPS = 193, 8


@pytest.fixture(scope="module")
def twin():
    """TEST-ONLY CPU build of the warm model solve and the car-by-car model loop (tests/host_twin, mpc_twin_solve / mpc_twin_rollout)."""
    return load_model_loop_twin()


@pytest.fixture(scope="module")
def fast(pkg, golden_dir):
    return pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))


@pytest.fixture(scope="module")
def pop(pkg, fast, waypoints):
    b, model = population(pkg, fast, waypoints, CARS)
    return b, model


@pytest.fixture(scope="module")
def loops(pkg, twin, fast, pop):
    """the car-by-car loops of the population in the three modes, computed once and left unchanged"""
    b, model = pop
    res = {}
    for mode, (warm_start, o) in MODES.items():
        res[mode] = twin_model_rollout(twin, fast, b, model, STEPS, pkg.warm_opts_default(**o), warm_start)
    return res


def _c_prototype(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


NEW = ("mpc_solve_batch_device_warm", "mpc_solve_batch_host_warm", "mpc_rollout_batch_device_warm", "mpc_rollout_batch_device_fused")


def test_abi(pkg):
    """The four prototypes are in the header -- each the entry point without `_model` plus `const double *model` directly behind
    `weights` -- the symbols are in the library with their argtypes set, a NULL handle gives -1 for each of them (with a model array
    and without), and the ABI version is still 5."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    header = open(os.path.join(_abi.ROOT, "include", "mpc_amd.h")).read()
    for name in NEW:
        base, got = _c_prototype(header, name), _c_prototype(header, name + "_model")
        at = base.index("const double *weights") + 1
        assert got == base[:at] + ["const double *model"] + base[at:], name
        assert hasattr(lib, name + "_model"), name
        fn, plain = getattr(lib, name + "_model"), getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(plain.argtypes[:at]) + [C.c_void_p] + list(plain.argtypes[at:]), name
    one = np.zeros(9); st = np.zeros(1, dtype=np.int32); m = np.ones((6, 1)); w = np.zeros((9 * 22, 1))
    p = lambda a: a.ctypes.data
    for model in (p(m), None):
        assert lib.mpc_solve_batch_device_warm_model(None, 1, 1, p(one), p(one), p(one), p(one), None, model, None, None, p(w), 1, None, p(one), None,
                                                     p(st), None, None) == -1
        assert lib.mpc_solve_batch_host_warm_model(None, 1, 1, p(one), p(one), p(one), p(one), None, model, None, None, p(w), 1, None, p(one), None,
                                                   p(st), None) == -1
        assert lib.mpc_rollout_batch_device_warm_model(None, 1, 1, 2, p(one), p(one), p(one), p(one), None, model, None, None, p(st), None, None) == -1
        for warm_start in (0, 1):
            assert lib.mpc_rollout_batch_device_fused_model(None, 1, 1, 2, p(one), p(one), p(one), p(one), None, model, warm_start, None, None,
                                                            p(st), None, None) == -1
        assert lib.mpc_last_error()
    assert lib.mpc_abi_version() == 5


@pytest.mark.parametrize("mode", list(MODES))
def test_uniform_rows_are_the_plain_twins_bitwise(pkg, twin, fast, pop, mode):
    """Rows equal to the handle's values: the car-by-car model loop is tests/host_twin (mpc_twin_rollout) and the closed loop of tests/host_twin (mpc_twin_solve) --
    hist, state and every solve's status and iterations."""
    b, _ = pop
    warm_start, o = MODES[mode]
    opts = pkg.warm_opts_default(**o)
    uni = pkg.scenarios.model_rows(fast, CARS)
    got = twin_model_rollout(twin, fast, b, uni, STEPS, opts, warm_start)
    plain = twin_rollout(load_rollout_twin(), fast, b, STEPS, opts, warm_start)
    for k in ("hist", "state", "status", "iters", "step_status", "step_iters"):
        assert np.array_equal(got[k], plain[k], equal_nan=True), (mode, k)
    hist, sst, sit = twin_closed_loop(load_warm_twin(), fast, b, STEPS, opts, warm_start=warm_start)
    assert np.array_equal(got["hist"], hist, equal_nan=True) and np.array_equal(got["state"], hist[-1, :6], equal_nan=True)
    assert np.array_equal(got["step_status"], sst) and np.array_equal(got["step_iters"], sit)
    step = twin_model_step_loop(twin, fast, b, uni, STEPS, opts, warm_start)
    assert np.array_equal(step["hist"], hist, equal_nan=True)


@pytest.mark.parametrize("mode", list(MODES))
def test_car_by_car_is_step_by_step_bitwise(pkg, twin, fast, pop, loops, mode):
    """193 cars x 8 steps with per-car rows: the loop over single warm model solves, warm buffer and status in place, against the
    car-by-car loop, and what the call reports per car is the fold of its steps."""
    b, model = pop
    warm_start, o = MODES[mode]
    step = twin_model_step_loop(twin, fast, b, model, STEPS, pkg.warm_opts_default(**o), warm_start)
    r = loops[mode]
    for k in ("hist", "state", "step_status", "step_iters"):
        assert np.array_equal(r[k], step[k], equal_nan=True), (mode, k)
    assert np.array_equal(r["status"], r["step_status"].max(0)) and np.array_equal(r["iters"], r["step_iters"].sum(0))
    # the rows matter: the loop with the handle's own values is another loop nearly everywhere
    uni = twin_model_rollout(twin, fast, b, pkg.scenarios.model_rows(fast, CARS), STEPS, pkg.warm_opts_default(**o), warm_start)
    assert (np.abs(uni["hist"][0, 6] - r["hist"][0, 6]) > 1e-4).sum() >= 150


@pytest.mark.parametrize("mode", ["warm", "warm_shift1"])
def test_warm_changes_the_iterate_not_the_answer(pop, loops, mode):
    """Every solve of the warm loop has the cold loop's status (so none that succeeds cold fails warm); on the cars both loops finish
    delta0, a0 and the step-1 state of every step are within the tolerances of the cold loop's; every 4th car follows the oracle's own
    cold loop; and from step 2 on the warm loop needs fewer iterations (0.39-0.51 of the cold ones on the CPU build)."""
    b, model = pop
    cold, warm = loops["cold"], loops[mode]
    assert np.array_equal(warm["step_status"], cold["step_status"])
    assert not ((cold["step_status"] == 0) & (warm["step_status"] != 0)).any()
    both = (cold["status"] == 0) & (warm["status"] == 0)
    assert both.sum() >= 150
    d_steer = np.abs(warm["hist"][:, 6, both] - cold["hist"][:, 6, both]).max(); d_acc = np.abs(warm["hist"][:, 7, both] - cold["hist"][:, 7, both]).max()
    d_state = np.abs(warm["hist"][:, :6, both] - cold["hist"][:, :6, both]).max()
    print("%s vs cold, %d cars x %d steps: max |d steer| %.3g rad, |d accel| %.3g, |d state| %.3g" % (mode, both.sum(), STEPS, d_steer, d_acc, d_state))
    assert d_steer <= TOL_STEER and d_acc <= TOL_ACCEL and d_state <= TOL_TRAJ
    ratio = warm["step_iters"][1:, both].sum() / cold["step_iters"][1:, both].sum()
    print("%s: iterations from step 2 on, warm / cold = %.3f" % (mode, ratio))
    assert ratio < 1
    cars = [i for i in range(0, CARS, 4)]
    orc = oracle_model_loops("config-fast.json", b, model, cars, STEPS)
    for name, r in (("cold", cold), (mode, warm)):
        assert_loops_follow_oracle(r["hist"], r["step_status"], orc, what=name)


def test_a_record_that_no_longer_fits_starts_cold(pkg, twin, fast, pop):
    """The records of a cold call go to a call whose max_steering row is halved.  A column that holds a |delta_k| above
    max_steering_i (1 + 1e-8) is refused by warm_point() and is bitwise the cold model solve, iterations included (16 of 176 on the
    CPU build); the others start warm; all statuses are the cold call's.  All-NaN and far-off records: the cold solve on every column."""
    b, model = pop
    opts = pkg.warm_opts_default()
    first = twin_warm_model_solve(twin, fast, b, model, opts)
    narrow = model.copy(); narrow[2] *= 0.5
    cold = twin_warm_model_solve(twin, fast, b, narrow, opts)
    got = twin_warm_model_solve(twin, fast, b, narrow, opts, warm=first["warm"], warm_status=first["status"])
    good = first["status"] == 0
    refused = good & steering_outside(fast.N, first["warm"], narrow[2])
    warm = good & ~refused
    print("halved max_steering: %d records refused, %d start warm, iterations warm / cold on those %.3f" %
          (refused.sum(), warm.sum(), got["iters"][warm].sum() / cold["iters"][warm].sum()))
    assert refused.sum() >= 8 and warm.sum() >= 8
    assert np.array_equal(got["status"], cold["status"])
    for k in ("out", "iters", "warm"):
        assert np.array_equal(got[k][..., refused], cold[k][..., refused]), k
        assert np.array_equal(got[k][..., ~good], cold[k][..., ~good]), k         # (no valid record: cold as well)
    # the others did start warm: fewer iterations in all, and not the cold solve's count nearly everywhere
    assert got["iters"][warm].sum() < cold["iters"][warm].sum() and (got["iters"][warm] != cold["iters"][warm]).sum() >= 8
    ok = warm & (cold["status"] == 0)
    assert np.abs(got["out"][6, ok] - cold["out"][6, ok]).max() <= TOL_STEER and np.abs(got["out"][7, ok] - cold["out"][7, ok]).max() <= TOL_ACCEL
    assert np.abs(got["out"][:6, ok] - cold["out"][:6, ok]).max() <= TOL_TRAJ
    cold_same = twin_warm_model_solve(twin, fast, b, model, opts)
    for spoilt in garbage_warm(fast, first["warm"]):
        g = twin_warm_model_solve(twin, fast, b, model, opts, warm=spoilt, warm_status=first["status"])
        for k in ("out", "status", "iters", "warm"):
            assert np.array_equal(g[k], cold_same[k]), k


def test_unusable_and_infeasible_columns(pkg, twin, fast, pop, loops):
    """A NaN dt and max_deceleration >= 0 in a warm loop: INFEASIBLE at every step, with finite outputs and no not-a-number in the
    warm buffer, and the neighbouring cars are bitwise what they are without them.  The 17 cars above their own speed limit are
    INFEASIBLE at their first step and are reported so; the start point they are reported with (v = 0) is their next state, from
    which step 2 starts cold -- bitwise the cold loop's step 2 -- and the loop goes on."""
    b, model = pop
    clean = loops["warm"]
    fastcars = np.where(clean["step_status"][0] == INFEASIBLE)[0]
    assert len(fastcars) == 17 and (np.abs(b["state"][3, fastcars]) > model[5, fastcars]).all()
    at = [int(i) for i in np.where(clean["status"] == 0)[0][[5, 40, 77, 120]]]
    spoilt = model.copy()
    spoilt[0, at[0]] = np.nan
    spoilt[4, at[1]] = 0.0
    spoilt[4, at[2]] = 2.5
    spoilt[:, at[3]] = np.nan
    opts = pkg.warm_opts_default()
    step = twin_model_step_loop(twin, fast, b, spoilt, STEPS, opts, True)
    car = twin_model_rollout(twin, fast, b, spoilt, STEPS, opts, True)
    for k in ("hist", "state", "step_status", "step_iters"):
        assert np.array_equal(step[k], car[k], equal_nan=True), k
    assert (step["step_status"][:, at] == INFEASIBLE).all(), step["step_status"][:, at]
    assert (step["step_iters"][:, at] == 0).all()
    # a car above its own speed limit is refused at its first step; the start point it is reported with becomes its next state
    assert (step["step_status"][0, fastcars] == INFEASIBLE).all() and (car["status"][fastcars] == INFEASIBLE).all()
    cold = loops["cold"]
    for k in ("hist", "step_status", "step_iters"):
        assert np.array_equal(step[k][:2][..., fastcars], cold[k][:2][..., fastcars]), k
    assert (step["hist"][0, 3, fastcars] == 0).all() and (step["step_status"][1:, fastcars] == 0).all()
    assert np.isfinite(step["hist"]).all() and np.isfinite(step["state"]).all() and np.isfinite(step["warm"]).all()
    rest = np.setdiff1d(np.arange(CARS), at)
    for k in ("hist", "state", "step_status", "step_iters"):
        assert np.array_equal(step[k][..., rest], clean[k][..., rest]), k
