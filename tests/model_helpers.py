"""Helpers of the per-instance model tests (test infrastructure): the TEST-ONLY CPU build (mpc_twin_solve of tests/host_twin), the population both test
files use, and the oracle solving every instance with its own OrcConfig -- the yardstick of these tests."""
import ctypes as C

import numpy as np

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, load_twin, vp

MODEL_FIELDS = ("dt", "Lf", "max_steering", "max_acceleration", "max_deceleration", "max_speed")   # rows of a model array
INFEASIBLE = 3   # MPC_STATUS_INFEASIBLE


load_model_twin = load_twin


def draw_rows(params, B, seed=5, dts=(0.05, 0.08, 0.1, 0.15)):
    """The rows of the stated population, drawn in the stated order."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([
        rng.choice(list(dts), B),
        rng.uniform(2.0, 3.5, B),
        rng.uniform(0.3, 0.5, B),
        rng.uniform(2.0, 5.0, B),
        -rng.uniform(3.0, 8.0, B),
        rng.uniform(0.6, 1.2, B) * params.max_speed]))


def population(pkg, params, waypoints, B=193):
    """lake_track_batch(B, seed 77) with the rows of draw_rows: (batch, model [6, B])."""
    b = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=77)
    b = {k: np.ascontiguousarray(b[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    return b, draw_rows(params, B)


def twin_model_solve(twin, params, batch, model, weights=None, want_traj=True):
    """Solver::setup / unpack of the device header on the instance's model column, CPU build, with the arguments of mpc_solve_batch_host_model."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh, md = f(batch["state"]), f(batch["coeffs"]), f(batch["yaw_lo"]), f(batch["yaw_hi"]), f(model)
    B = st.shape[1]
    assert md.shape == (6, B)
    out = np.zeros((9, B)); traj = np.zeros((2 * params.N, B)) if want_traj else None
    status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    w = f(weights) if weights is not None else None
    rc = twin.mpc_twin_solve(C.byref(params), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), vp(w), vp(md), None, None, None,
                             C.c_int64(0), None, C.c_int(0), vp(out), vp(traj), vp(status), vp(iters))
    assert rc == 0
    return {"out": out, "traj": traj, "status": status, "iters": iters}


def oracle_model_solve(cfgname, batch, model, idx=None, **overrides):
    """The oracle on the selected instances (default: all), each with its own OrcConfig: dt, Lf and the limits of its column."""
    idx = range(batch["state"].shape[1]) if idx is None else idx
    n = len(idx)
    N = O.load_config(cfgname, **overrides).N
    out = np.zeros((9, n)); traj = np.zeros((2 * N, n)); status = np.zeros(n, dtype=np.int32); iters = np.zeros(n, dtype=np.int32)
    for j, i in enumerate(idx):
        over = dict(overrides)
        over.update({name: float(model[q, i]) for q, name in enumerate(MODEL_FIELDS)})
        cfg = O.load_config(cfgname, **over)
        cfg.yaw_low, cfg.yaw_high = float(batch["yaw_lo"][i]), float(batch["yaw_hi"][i])
        st, o9, tx, ty, info = O.mpc_solve(cfg, batch["state"][:, i], batch["coeffs"][:, i])
        out[:, j] = o9; traj[:N, j] = tx; traj[N:, j] = ty; status[j] = st; iters[j] = info.iterations
    return {"out": out, "traj": traj, "status": status, "iters": iters}


def assert_matches_oracle(got, ref, idx=None, what=""):
    """The stated conditions: the oracle's status on every instance, and every instance it converges on within the three
    tolerances (delta0, a0, step-1 state and -- where both sides have them -- the trajectory points); none left out."""
    idx = np.arange(ref["status"].shape[0]) if idx is None else np.asarray(idx)
    gs = got["status"][idx]
    assert np.array_equal(gs, ref["status"]), (what, "status differs at", idx[gs != ref["status"]][:8].tolist(), gs[gs != ref["status"]][:8].tolist(),
                                               ref["status"][gs != ref["status"]][:8].tolist())
    ok = ref["status"] == 0
    go = got["out"][:, idx]
    d_steer = np.abs(go[6, ok] - ref["out"][6, ok]).max(); d_acc = np.abs(go[7, ok] - ref["out"][7, ok]).max()
    d_state = np.abs(go[:6, ok] - ref["out"][:6, ok]).max()
    d_traj = 0.0
    if got.get("traj") is not None and ref.get("traj") is not None:
        d_traj = np.abs(got["traj"][:, idx][:, ok] - ref["traj"][:, ok]).max()
    print("%s vs oracle: %d converged of %d, max |d steer| %.3g rad, |d accel| %.3g, |d state| %.3g, |d traj| %.3g" %
          (what, int(ok.sum()), len(idx), d_steer, d_acc, d_state, d_traj))
    assert d_steer <= TOL_STEER and d_acc <= TOL_ACCEL and d_state <= TOL_TRAJ and d_traj <= TOL_TRAJ, (what, d_steer, d_acc, d_state, d_traj)
    assert np.isfinite(got["out"]).all(), what
