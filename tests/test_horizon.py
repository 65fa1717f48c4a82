"""Per-instance horizon (include/mpc_amd_horizon.h: the seven mpc_*_horizon entry points), checked without a GPU: the CPU build
tests/host_twin/horizon_twin.cpp runs the per-instance driver of csrc/mpc_core.h with an mpc::HorizonColumn -- the
Solver::setup / solve_warm / warm_store / unpack (on an mpc::HorizonColumn) and mpc::RolloutCar that the HORIZON builds of the lane kernel
run per lane.  Yardsticks: the existing twin on handles created with N = n (bitwise), and the oracle with one OrcConfig of
N = n_i per instance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, closed_loop_report, load_twin
from horizon_helpers import (INFEASIBLE, LOOP_HORIZONS, SENTINEL, WARM_REC, assert_columns_equal_per_n, draw_horizons, judge_n_dt,
                             load_horizon_twin, masked_traj, n_dt_study, oracle_horizon_solve, oracle_loops_per_group, stated_population,
                             sub_batch, twin_horizon_rollout, twin_horizon_solve, twin_horizon_step_loop, twin_plain_solve, with_N)
from model_helpers import assert_matches_oracle

FORMS = {  # the _horizon form -> its _model form
    "mpc_solve_batch_device_horizon": "mpc_solve_batch_device_model",
    "mpc_solve_batch_host_horizon": "mpc_solve_batch_host_model",
    "mpc_solve_batch_device_warm_horizon": "mpc_solve_batch_device_warm_model",
    "mpc_solve_batch_host_warm_horizon": "mpc_solve_batch_host_warm_model",
    "mpc_rollout_batch_device_horizon": "mpc_rollout_batch_device_model",
    "mpc_rollout_batch_device_warm_horizon": "mpc_rollout_batch_device_warm_model",
    "mpc_rollout_batch_device_fused_horizon": "mpc_rollout_batch_device_fused_model",
}


@pytest.fixture(scope="module")
def twin():
    return load_horizon_twin()


@pytest.fixture(scope="module")
def plain():
    """the existing twin (tests/host_twin, mpc_twin_solve): handles created with N = n"""
    return load_twin()


@pytest.fixture(scope="module")
def pop(pkg, golden_dir, waypoints):
    return stated_population(pkg, golden_dir, waypoints)


@pytest.fixture(scope="module")
def cold(pkg, twin, pop):
    """the stated batch, cold, with traj and warm_out: computed once and left unchanged"""
    params, b, model, horizon = pop
    return twin_horizon_solve(twin, params, b, horizon, pkg.warm_opts_default(), model=model, want_warm=True)


def _c_prototype(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_abi(pkg):
    """The seven prototypes are in the header (include/mpc_amd_horizon.h, which mpc_amd.h includes), each its _model form plus
    `const int32_t *horizon` directly behind `model`; the symbols are in the library with argtypes that say the same; a NULL handle
    is refused by every form; the ABI version is 5."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    inc = os.path.join(_abi.ROOT, "include")
    assert '#include "mpc_amd_horizon.h"' in open(os.path.join(inc, "mpc_amd.h")).read()      # (the section's own file, part of mpc_amd.h)
    header = open(os.path.join(inc, "mpc_amd.h")).read() + open(os.path.join(inc, "mpc_amd_horizon.h")).read()
    assert sorted(FORMS) == sorted(_abi.HORIZON_EXPORTS)
    for name, model_form in FORMS.items():
        base, got = _c_prototype(header, model_form), _c_prototype(header, name)
        at = base.index("const double *model") + 1
        assert got == base[:at] + ["const int32_t *horizon"] + base[at:], name
        assert hasattr(lib, name), name
        fn, mf = getattr(lib, name), getattr(lib, model_form)
        assert fn.argtypes is not None and list(fn.argtypes) == list(mf.argtypes[:at]) + [C.c_void_p] + list(mf.argtypes[at:]), name
    one = np.zeros(9); st = np.zeros(1, dtype=np.int32); m = np.ones((6, 1)); w = np.zeros((9 * 22, 1)); hz = np.full(1, 5, dtype=np.int32)
    p = lambda a: a.ctypes.data
    for model in (p(m), None):
        for horizon in (p(hz), None):
            assert lib.mpc_solve_batch_device_horizon(None, 1, 1, p(one), p(one), p(one), p(one), None, model, horizon, p(one), None, p(st), None, None) == -1
            assert lib.mpc_solve_batch_host_horizon(None, 1, 1, p(one), p(one), p(one), p(one), None, model, horizon, p(one), None, p(st), None) == -1
            assert lib.mpc_solve_batch_device_warm_horizon(None, 1, 1, p(one), p(one), p(one), p(one), None, model, horizon, None, None, p(w), 1, None,
                                                           p(one), None, p(st), None, None) == -1
            assert lib.mpc_solve_batch_host_warm_horizon(None, 1, 1, p(one), p(one), p(one), p(one), None, model, horizon, None, None, p(w), 1, None,
                                                         p(one), None, p(st), None) == -1
            assert lib.mpc_rollout_batch_device_horizon(None, 1, 1, 2, p(one), p(one), p(one), p(one), None, model, horizon, None, p(st), None, None) == -1
            assert lib.mpc_rollout_batch_device_warm_horizon(None, 1, 1, 2, p(one), p(one), p(one), p(one), None, model, horizon, None, None, p(st),
                                                             None, None) == -1
            for warm_start in (0, 1):
                assert lib.mpc_rollout_batch_device_fused_horizon(None, 1, 1, 2, p(one), p(one), p(one), p(one), None, model, horizon, warm_start, None,
                                                                  None, p(st), None, None) == -1
            assert lib.mpc_last_error()
    assert lib.mpc_abi_version() == 5


def test_cold_columns_are_those_of_handles_of_that_N_bitwise(pkg, plain, pop, cold):
    """B = 193, horizons from {3,4,5,7,10,13,17,25} on an N = 25 handle: every column is the existing twin's on a handle created with
    N = n_i -- out, status, iters, the trajectory prefix, the warm_out prefix -- and the sentinel stands behind the prefixes."""
    params, b, model, horizon = pop
    opts = pkg.warm_opts_default()
    assert set(horizon.tolist()) == {3, 4, 5, 7, 10, 13, 17, 25}
    assert_columns_equal_per_n(cold, params.N, horizon,
                               lambda n, idx: twin_plain_solve(plain, with_N(params, n), sub_batch(b, idx), opts, model=model[:, idx], want_warm=True), "cold")
    assert (cold["status"] == 0).sum() > 150


def test_no_model_is_the_handles_own_values_bitwise(pkg, twin, plain, pop):
    """model = NULL with a horizon: the handle's six values, bitwise the plain call (no `model`) of a handle created with N = n."""
    params, b, _, horizon = pop
    got = twin_horizon_solve(twin, params, b, horizon)
    assert got["warm"] is None
    assert_columns_equal_per_n(got, params.N, horizon, lambda n, idx: twin_plain_solve(plain, with_N(params, n), sub_batch(b, idx)), "no model")


@pytest.mark.parametrize("shift", (0, 1))
def test_warm_columns_are_those_of_handles_of_that_N_bitwise(pkg, twin, plain, pop, cold, shift):
    """The warm call from the cold call's records and status (the rows behind an instance's records hold the sentinel: a solve that
    read them would refuse the record and count a cold solve's iterations), shift 0 and 1 -- with shift 1 the repeated record is
    record n - 2 -- against handles created with N = n warm-started from their own cold call."""
    params, b, model, horizon = pop
    opts = pkg.warm_opts_default(shift=shift)
    got = twin_horizon_solve(twin, params, b, horizon, opts, model=model, warm=cold["warm"], warm_status=cold["status"])

    def ref_of(n, idx):
        pn, sb = with_N(params, n), sub_batch(b, idx)
        c = twin_plain_solve(plain, pn, sb, opts, model=model[:, idx], want_warm=True)
        return twin_plain_solve(plain, pn, sb, opts, model=model[:, idx], warm=c["warm"], warm_status=c["status"])
    assert_columns_equal_per_n(got, params.N, horizon, ref_of, "warm shift %d" % shift)
    ok = cold["status"] == 0
    assert got["iters"][ok].sum() < cold["iters"][ok].sum()          # (it did start warm)
    assert np.array_equal(got["iters"][~ok], cold["iters"][~ok])      # only SUCCESS columns start warm: the others are the cold solve


def test_every_instance_against_the_oracle(pop, cold):
    """One OrcConfig with N = n_i per instance: the oracle's status on every instance, the three tolerances on every converged one."""
    params, b, model, horizon = pop
    ref = oracle_horizon_solve("config-fast.json", b, model, horizon, params.N)
    assert (ref["status"] == 0).sum() > 150 and (ref["status"] == INFEASIBLE).sum() > 0
    assert_matches_oracle(masked_traj(cold, params.N, horizon), ref, what="horizon twin")


@pytest.fixture(scope="module")
def loops(pkg, twin, golden_dir, waypoints):
    """96 cars x 25 steps (config-fast.json at N = 25, seed 122), horizons from {3,4,5,7,10}: car by car, cold and warm, and the
    oracle's own loops with N = n per group.  Computed once."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), N=25)
    cars, steps = 96, 25
    sc = pkg.scenarios.lake_track_batch(cars, params, waypoints, seed=122)
    sc = {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    horizon = draw_horizons(cars, seed=11, choices=LOOP_HORIZONS)
    opts = pkg.warm_opts_default()
    res = {"params": params, "sc": sc, "horizon": horizon, "steps": steps, "opts": opts}
    res["cold"] = twin_horizon_rollout(twin, params, sc, horizon, steps, opts, False)
    res["warm"] = twin_horizon_rollout(twin, params, sc, horizon, steps, opts, True)
    res["oracle"] = oracle_loops_per_group("config-fast.json", sc, horizon, steps)
    return res


@pytest.mark.parametrize("mode", ("cold", "warm"))
def test_closed_loops_match_the_oracle(loops, mode):
    r = loops[mode]
    oh, ost = loops["oracle"]
    assert set(loops["horizon"].tolist()) == set(LOOP_HORIZONS)
    cl = closed_loop_report(r["hist"], r["step_status"], oh, ost)
    print("%s closed loops vs oracle: status differs %d, forks %d, max |d steer| %.3g rad, |d accel| %.3g, |d state| %.3g" %
          (mode, cl["status_differs"], cl["cars_on_another_local_minimum"], cl["d_steer_rad"][3], cl["d_accel"][3], cl["d_state"][3]))
    assert cl["status_differs"] == 0 and cl["cars_on_another_local_minimum"] == 0, cl
    assert cl["d_steer_rad"][3] <= TOL_STEER and cl["d_accel"][3] <= TOL_ACCEL and cl["d_state"][3] <= TOL_TRAJ, cl


def test_warm_loops_save_iterations(loops):
    cold_it, warm_it = int(loops["cold"]["step_iters"][1:].sum()), int(loops["warm"]["step_iters"][1:].sum())
    print("iterations, steps 2..25: cold %d, warm %d, ratio %.3f" % (cold_it, warm_it, warm_it / cold_it))
    assert warm_it < cold_it


@pytest.mark.parametrize("mode", ("cold", "warm"))
def test_car_by_car_is_step_by_step_bitwise(twin, loops, mode):
    """the loop of whole-batch solves, the warm buffer handed on, against the car-by-car loop (8 steps)"""
    steps = 8
    step = twin_horizon_step_loop(twin, loops["params"], loops["sc"], loops["horizon"], steps, loops["opts"], mode == "warm")
    r = loops[mode]
    for k in ("hist", "step_status", "step_iters"):
        assert np.array_equal(r[k][:steps], step[k], equal_nan=True), (mode, k)


def test_the_reference_n_dt_study_as_one_batch(pkg, twin, golden_dir):
    """The 14 N / dt figures as 14 columns of ONE batch on an N = 50 handle: dt from the model row, N from `horizon`, 26 steps,
    judged exactly as test_twin_reproduces_every_n_dt_figure judges its 14 handles."""
    entries, params, sc, W, model, horizon, pre = n_dt_study(pkg, golden_dir)
    assert len(entries) == 14
    r = twin_horizon_rollout(twin, params, sc, horizon, 26, pkg.warm_opts_default(), False, model=model, weights=W)
    judge_n_dt(entries, r["hist"], r["step_status"].max(0), pre)


def test_unusable_horizons(pkg, twin, pop, cold):
    """2, 0, -1 and N + 1 scattered over the batch: MPC_STATUS_INFEASIBLE with finite outputs, every other column bitwise what it is
    without them."""
    params, b, model, horizon = pop
    bad = {5: 2, 64: 0, 100: -1, 192: params.N + 1}
    hz = horizon.copy()
    for i, v in bad.items():
        hz[i] = v
    got = twin_horizon_solve(twin, params, b, hz, pkg.warm_opts_default(), model=model, want_warm=True)
    at = np.array(sorted(bad))
    keep = np.setdiff1d(np.arange(hz.shape[0]), at)
    assert (got["status"][at] == INFEASIBLE).all() and (got["iters"][at] == 0).all()
    assert np.isfinite(got["out"]).all()
    for k in ("out", "status", "iters", "traj", "warm"):
        assert np.array_equal(got[k][..., keep], cold[k][..., keep], equal_nan=True), k
    # the start point in `out`: the state the handle's own horizon would start from, nothing moved
    assert np.array_equal(got["out"][6:8, at], np.zeros((2, at.size)))
