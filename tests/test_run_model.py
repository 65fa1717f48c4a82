"""run() and the telemetry handler with per-instance model values, on the CPU: tests/host_twin (mpc_twin_run) -- the templated run_pre /
telemetry_to_pose / run_post / command_from_run of csrc/mpc_run_core.h around Solver::setup / solve_warm / unpack (on the instance's model column), built
with g++ -- against the oracle's mpc_run / telemetry_handler with a per-car OrcConfig on the stated population (48 lake-track cars,
seed 77, the columns of draw_rows seed 9), against tests/host_twin (mpc_twin_run without a model array) for columns that repeat the handle's values, and on columns
that cannot be used."""
import os

import numpy as np
import pytest

from run_model_helpers import (EXTRA_LATENCY, FLEET_B, INFEASIBLE, assert_fleet_matches_oracle, assert_pre_matches_oracle, fleet, load_run_model_twin,
                               oracle_fleet, twin_run_model, uniform_model)
from run_warm_helpers import load_run_warm_twin, twin_run


@pytest.fixture(scope="module")
def twin():
    return load_run_model_twin()


@pytest.fixture(scope="module")
def warm_twin():
    return load_run_warm_twin()


@pytest.mark.parametrize("cfgname", ["config-fast.json", "config-stable.json"])
def test_twin_follows_the_oracle_with_a_config_per_car(pkg, twin, golden_dir, waypoints, cfgname):
    """run() and the telemetry handler, every car with its own dt, Lf and limits: the oracle's status on all 48, every car it
    converges on within the tolerances, `pre` and the vehicle-frame waypoints as the oracle's run() derives them.  A call that
    ignored the columns could not pass: against the handle's own config the oracle's replies differ by up to 0.54 (steering) and
    1.97 (throttle)."""
    params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
    F = fleet(pkg, params, waypoints)
    opts = pkg.warm_opts_default()
    run = twin_run_model(twin, params, F["pose"], F["ptsx"], F["ptsy"], F["model"], opts)
    ref = oracle_fleet(cfgname, F["pose"], F["ptsx"], F["ptsy"], F["model"])
    print("%s: oracle SUCCESS %d, INFEASIBLE %d, most iterations %d" % (cfgname, (ref["status"] == 0).sum(), (ref["status"] == INFEASIBLE).sum(),
                                                                         ref["iters"][ref["status"] == 0].max()))
    # the cars the oracle refuses are those faster than their own speed limit
    assert np.array_equal(ref["status"] == INFEASIBLE, F["pose"][3] > F["model"][5] * (1 + 1e-8))
    assert_fleet_matches_oracle(run, ref, F["model"], what="run(), " + cfgname)
    assert_pre_matches_oracle(run, ref, what="run(), " + cfgname)
    tel = twin_run_model(twin, params, F["tel"], F["ptsx"], F["ptsy"], F["model"], opts, tel=True, extra=EXTRA_LATENCY)
    tref = oracle_fleet(cfgname, F["tel"], F["ptsx"], F["ptsy"], F["model"], tel=True, extra=EXTRA_LATENCY)
    assert np.array_equal(tref["status"] == 0, ref["status"] == 0)          # the handler gives the same split
    assert_fleet_matches_oracle(tel, tref, F["model"], tel=True, what="telemetry, " + cfgname)
    # ... and the columns matter: the same calls with the handle's values in every column are elsewhere
    plain = twin_run_model(twin, params, F["tel"], F["ptsx"], F["ptsy"], uniform_model(params, FLEET_B), opts, tel=True, extra=EXTRA_LATENCY)
    assert np.abs(plain["cmd"] - tel["cmd"]).max() > 0.1


@pytest.mark.parametrize("tel", [False, True])
def test_uniform_columns_are_the_run_warm_twin_bitwise(pkg, twin, warm_twin, golden_dir, waypoints, tel):
    """every column the handle's own values: bitwise tests/host_twin (mpc_twin_run without a model array), cold and warm"""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    F = fleet(pkg, params, waypoints)
    opts = pkg.warm_opts_default()
    model = uniform_model(params, FLEET_B)
    rows = F["tel"] if tel else F["pose"]
    extra = EXTRA_LATENCY if tel else 0.0
    a = twin_run_model(twin, params, rows, F["ptsx"], F["ptsy"], model, opts, tel=tel, extra=extra)
    b = twin_run(warm_twin, params, rows, F["ptsx"], F["ptsy"], opts, tel=tel, extra=extra)
    keys = ("out8", "cmd", "status", "iters", "pre", "warm")
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), ("cold", k)
    assert (a["status"] == 0).sum() >= 40
    # the next message of every car (its pose moved a little along its heading), warm-started from that record
    nxt = rows.copy()
    nxt[0] += 0.3 * np.cos(rows[2]); nxt[1] += 0.3 * np.sin(rows[2])
    a2 = twin_run_model(twin, params, nxt, F["ptsx"], F["ptsy"], model, opts, warm=a["warm"], warm_status=a["status"], tel=tel, extra=extra)
    b2 = twin_run(warm_twin, params, nxt, F["ptsx"], F["ptsy"], opts, warm=b["warm"], warm_status=b["status"], tel=tel, extra=extra)
    for k in keys:
        assert np.array_equal(a2[k], b2[k], equal_nan=True), ("warm", k)
    assert a2["iters"].sum() < a["iters"].sum()


def test_an_unusable_column_ends_infeasible_and_leaves_its_neighbours_alone(pkg, twin, golden_dir, waypoints):
    """NaN, dt = 0 and max_deceleration = 0, one car each: INFEASIBLE with finite out8, cmd, pre and warm record; every other car is
    bitwise what it was, cold and warm."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    F = fleet(pkg, params, waypoints)
    opts = pkg.warm_opts_default()
    good = twin_run_model(twin, params, F["tel"], F["ptsx"], F["ptsy"], F["model"], opts, tel=True, extra=EXTRA_LATENCY)
    ok = np.where(good["status"] == 0)[0]
    bad_cars = ok[[1, 7, 20]]
    model = F["model"].copy()
    model[1, bad_cars[0]] = np.nan; model[0, bad_cars[1]] = 0.0; model[4, bad_cars[2]] = 0.0
    others = np.setdiff1d(np.arange(FLEET_B), bad_cars)
    keys = ("out8", "cmd", "status", "iters", "pre", "warm")
    for warm, wst in ((None, None), (good["warm"], good["status"])):
        r = twin_run_model(twin, params, F["tel"], F["ptsx"], F["ptsy"], model, opts, warm=warm, warm_status=wst, tel=True, extra=EXTRA_LATENCY)
        ref = good if warm is None else twin_run_model(twin, params, F["tel"], F["ptsx"], F["ptsy"], F["model"], opts, warm=warm, warm_status=wst, tel=True,
                                                       extra=EXTRA_LATENCY)
        assert (r["status"][bad_cars] == INFEASIBLE).all()
        for k in keys:
            assert np.isfinite(r[k][..., bad_cars]).all(), k
            assert np.array_equal(r[k][..., others], ref[k][..., others]), k
