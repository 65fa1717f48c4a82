"""Every CPU solve path against the EXACT minimisers of tests/golden/exact_minimisers.npz (tests/golden/make_exact_minimisers.py:
the NLP restated from MPC.cpp and the headers' words, solved in 70-digit arithmetic with differenced derivatives only).

The oracle first -- its distance to the exact values IS the yardstick (8 x its class maximum), so this checks the fixture and the
harness -- then the CPU twin through every entry point the suite has, the two SLSQP files within their own stated tolerances, and
the certify twin at stored exact primal-dual points.  No case is left out anywhere.

Findings written down where they are asserted:
  * a speed bound that is active with strict complementarity does not exist in this NLP on an unmodified config (the generator's
    candidates() explains why), so the fixture has no `v_bound` class, and `a_free` runs on handles whose max_speed is raised above
    the speed table after the load;
  * an exact point that sits on the caller's bounds is not CONVERGED by the header's own rule: complementarity is measured against
    the relaxed bounds (see test_certify_twin_at_exact_points)."""
import os

import numpy as np
import pytest

import oracle_lib as O
from exact_helpers import (MEASURED, assert_certificates, assert_exact, fixture, group_params, record_groups, twin_paths)
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, load_golden
from model_helpers import MODEL_FIELDS

TWIN_PATHS = ("twin plain", "twin weights", "twin horizons", "twin f64_f32_start", "twin _model", "twin _horizon", "twin _warm", "twin _warm_model")


def test_fixture_holds_what_the_generator_asserts(pkg):
    fx = fixture()
    a = fx.a
    assert 6 * len(fx.classes) <= fx.n <= 160
    for cls in fx.classes:
        assert len(fx.of_class(cls)) >= 6, cls
        y = fx.yard[cls]
        assert y["steer"] <= TOL_STEER and y["accel"] <= TOL_ACCEL and y["state"] <= TOL_TRAJ and y["traj"] <= TOL_TRAJ, (cls, y)
        e = a["ref_err"][:, fx.of_class(cls)]
        assert 8 * e[6].max() <= y["steer"] and 8 * e[7].max() <= y["accel"] and 8 * e[:6].max() <= y["state"] and 8 * e[9].max() <= y["traj"], cls
    assert (a["margins"][0] >= 1e-3).all() and (a["margins"][1] >= 1e-5).all() and (a["margins"][2] > 0).all()
    assert len(fx.of_class("plain")) == len(load_golden("scipy_cross_solve.json")["cases"])
    # the model class as stated: a_0 on the column's max_acceleration on both sides of the handle's, delta_0 on the column's max_steering,
    # a column max_speed below the handle's
    m = fx.of_class("model")
    own = group_params(pkg, fx.groups("model")[0])
    on_amax = [i for i in m if a["act"][3, 0, i] == 1 and a["out"][7, i] == a["model"][3, i]]
    handle_amax = own.max_acceleration
    assert sum(a["model"][3, i] < handle_amax for i in on_amax) >= 2 and sum(a["model"][3, i] > handle_amax for i in on_amax) >= 2
    assert sum(a["act"][2, 0, i] != 0 and abs(a["out"][6, i]) == a["model"][2, i] for i in m) >= 4
    assert sum(a["model"][5, i] < own.max_speed for i in m) >= 2
    # a_free: all nine accelerations free; the other classes of the project's usual active set have a_0 on its bound
    for i in fx.of_class("a_free"):
        assert (a["act"][3, :, i] == 0).all()
    psi_active = [bool((a["act"][0, :, i] != 0).any()) for i in fx.of_class("plain")]
    print("plain: %d cases with an active psi bound, %d without" % (sum(psi_active), len(psi_active) - sum(psi_active)))
    assert sum(psi_active) >= 6 and len(psi_active) - sum(psi_active) >= 6


def _oracle_on(g):
    """the oracle on a group, every instance with its own OrcConfig (the options the handle's parameter set implies: the defaults)"""
    n = len(g["idx"])
    N = g["N"]
    out = np.zeros((9, n)); traj = np.zeros((2 * N, n)); status = np.zeros(n, dtype=np.int32)
    for j in range(n):
        over = {"N": int(g["horizon"][j]) if g["horizon"] is not None else N, "dt": g["dt"]}
        if g["max_speed"] is not None:
            over["max_speed"] = g["max_speed"]
        if g["model"] is not None:
            over.update({k: float(g["model"][q, j]) for q, k in enumerate(MODEL_FIELDS)})
        cfg = O.load_config(g["config"], **over)
        cfg.yaw_low, cfg.yaw_high = float(g["batch"]["yaw_lo"][j]), float(g["batch"]["yaw_hi"][j])
        if g["weights"] is not None:
            for q in range(12):
                cfg.weights[q] = float(g["weights"][q, j])
        st, o9, tx, ty, _ = O.mpc_solve(cfg, g["batch"]["state"][:, j], g["batch"]["coeffs"][:, j])
        k = over["N"]
        out[:, j] = o9; traj[:k, j] = tx; traj[N:N + k, j] = ty; status[j] = st
    return {"out": out, "traj": traj, "status": status}


def test_oracle_lies_within_its_own_yardsticks():
    """The oracle's distance to the exact values is what the fixture records as ref_err (to the rounding of another build of the
    oracle), and so lies within every yardstick: the harness (grouping, trajectory layout, the relative cost) and the fixture agree."""
    fx = fixture()
    for cls in fx.classes:
        for g in fx.groups(cls):
            r = _oracle_on(g)
            assert_exact(g, r, "oracle")
            e = fx.a["ref_err"][:, g["idx"]]
            d = np.abs(r["out"] - fx.a["out"][:, g["idx"]])
            assert (d <= 2 * e[:9] + 1e-13 * np.maximum(1.0, np.abs(fx.a["out"][:, g["idx"]]))).all(), cls


@pytest.mark.parametrize("path", TWIN_PATHS)
def test_twin_path(pkg, path):
    """The CPU build of the device header through the entry point `path` names, on every class that entry point serves."""
    paths = twin_paths(pkg)
    assert set(paths) == set(TWIN_PATHS)
    paths[path]()
    assert any(p.startswith(path) for p in MEASURED)


def test_slsqp_files_lie_within_their_stated_tolerances_of_the_exact_answers():
    """tests/golden/scipy_cross_solve.json (stated: 2e-6 on delta_0 and a_0, 2e-5 on the step-1 state) and scipy_cross_solve_ext.json
    (5e-6, 5e-5) against the exact minimisers of the same inputs; nothing in those files changes."""
    fx = fixture()
    a = fx.a
    by_name = {n: i for i, n in enumerate(fx.names)}
    worst = {}
    for fname, tol_u, tol_s, must_all in (("scipy_cross_solve.json", 2e-6, 2e-5, True), ("scipy_cross_solve_ext.json", 5e-6, 5e-5, False)):
        seen = 0
        for c in load_golden(fname)["cases"]:
            if c["name"] not in by_name:
                assert not must_all, c["name"]          # (the generator's admission test rejected it; it prints which)
                continue
            i = by_name[c["name"]]
            assert np.array_equal(a["state"][:, i], c["state"]) and np.array_equal(a["coef"][:, i], c["coef"]), c["name"]
            d = np.abs(np.array(c["out9"]) - a["out"][:, i])
            assert d[6] <= tol_u and d[7] <= tol_u and d[:6].max() <= tol_s, (fname, c["name"], d.tolist())
            w = worst.setdefault(fname, np.zeros(3))
            worst[fname] = np.maximum(w, [d[6], d[7], d[:6].max()])
            seen += 1
        assert seen >= (37 if must_all else 12), (fname, seen)
        print("%s: %d cases, SLSQP vs exact: d_steer %.3g d_accel %.3g d_state %.3g" % ((fname, seen) + tuple(worst[fname])))


def test_certify_twin_at_exact_points(pkg):
    """mpc_certify_twin at 24 exact primal-dual points and at their perturbed copies, every row against the generator's 70-digit
    value with the rounding bounds of certify_helpers.assert_rows.  The verdict is the one the header's rule gives on the exact rows:
    CONVERGED where no bound is active (the a_free records); where a quantity sits on the caller's bound, its slack against the
    RELAXED bound is bound_relax_factor max(1, |b|), slack x dual puts E_0 at 1e-8 .. 2e-6, and the verdict is ACCEPTABLE or
    NOT_CONVERGED -- at a point that is the minimiser to 16 digits.  Every perturbed copy is NOT_CONVERGED."""
    from certify_helpers import CONVERGED, NOT_CONVERGED, load_certify_twin, twin_certify
    twin = load_certify_twin()
    seen = set()
    for g in record_groups():
        p = group_params(pkg, g)
        assert_certificates(g, lambda sol: twin_certify(twin, p, g["batch"], sol, weights=g["weights"], model=g["model"], horizon=g["horizon"]),
                            "certify twin")
        assert (g["verdict"][1] == NOT_CONVERGED).all()
        if g["cls"] == "a_free":
            assert (g["verdict"][0] == CONVERGED).all()
        seen.add((g["cls"], g["N"]))
    assert {("plain", 10), ("a_free", 10), ("model", 10), ("horizons", 3), ("horizons", 25)} <= seen


if __name__ == "__main__":
    raise SystemExit(pytest.main([os.path.abspath(__file__), "-q", "-s"]))
