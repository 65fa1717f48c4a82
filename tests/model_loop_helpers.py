"""Helpers of the tests of warm starts and closed loops with per-instance model values (test infrastructure): the TEST-ONLY CPU build
(mpc_twin_solve and mpc_twin_rollout of tests/host_twin), the loops both test files run, and the oracle's own cold loop of one car with its own OrcConfig."""
import ctypes as C

import numpy as np

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, load_twin, vp
from model_helpers import MODEL_FIELDS

MODES = {"cold": (False, {}), "warm": (True, {}), "warm_shift1": (True, {"shift": 1})}
WARM_REC = 22


load_model_loop_twin = load_twin


def twin_warm_model_solve(twin, params, batch, model, opts, warm=None, warm_status=None, inplace=False, weights=None, want_traj=False):
    """One warm model solve, CPU build, with the arguments of mpc_solve_batch_host_warm_model.  inplace: warm_out is the `warm` array
    itself and the status is written into `warm_status`."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh, md = f(batch["state"]), f(batch["coeffs"]), f(batch["yaw_lo"]), f(batch["yaw_hi"]), f(model)
    B = st.shape[1]
    rows = (params.N - 1) * WARM_REC
    assert md.shape == (6, B)
    out = np.zeros((9, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    traj = np.zeros((2 * params.N, B)) if want_traj else None
    if warm is not None:
        warm = warm if inplace else f(warm).copy()
        assert warm.shape == (rows, B) and warm.flags.c_contiguous and warm.dtype == np.float64
    wout = warm if inplace else np.zeros((rows, B))
    if inplace and warm_status is not None:
        status = warm_status
    elif warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    w = f(weights) if weights is not None else None
    rc = twin.mpc_twin_solve(C.byref(params), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), vp(w), vp(md), vp(warm),
                             vp(warm_status), vp(wout), C.c_int64(B), C.byref(opts), C.c_int(0), vp(out), vp(traj), vp(status), vp(iters))
    assert rc == 0
    return {"out": out, "traj": traj, "status": status, "iters": iters, "warm": wout}


def twin_model_step_loop(twin, params, sc, model, steps, opts, warm_start, weights=None):
    """Step by step: `steps` warm model solves per batch, the warm buffer and its status in place (src/test.cpp:79-111 feeds the next
    state) -> hist [steps, 9, B], the final state, status and iterations of every solve [steps, B], and the warm buffer at the end."""
    B = sc["state"].shape[1]
    hist = np.zeros((steps, 9, B)); sst = np.zeros((steps, B), dtype=np.int32); sit = np.zeros((steps, B), dtype=np.int32)
    st = np.array(sc["state"], dtype=np.float64, copy=True)
    warm = np.zeros(((params.N - 1) * WARM_REC, B)); wstat = np.zeros(B, dtype=np.int32)
    for k in range(steps):
        first = k == 0 or not warm_start
        r = twin_warm_model_solve(twin, params, dict(sc, state=st), model, opts, warm=None if first else warm,
                                  warm_status=None if first else wstat, inplace=not first, weights=weights)
        if first:
            warm, wstat = r["warm"], r["status"].copy()
        hist[k] = r["out"]; sst[k] = r["status"]; sit[k] = r["iters"]
        st = r["out"][:6].copy()
    return {"hist": hist, "state": st, "step_status": sst, "step_iters": sit, "warm": warm}


def twin_model_rollout(twin, params, sc, model, steps, opts, warm_start, weights=None):
    """Car by car through mpc::RolloutCar (the arguments of mpc_rollout_batch_device_fused_model) -> hist [steps, 9, B], the final state,
    worst status and summed iterations [B], status and iterations of every solve [steps, B]."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh, md = f(sc["state"]).copy(), f(sc["coeffs"]), f(sc["yaw_lo"]), f(sc["yaw_hi"]), f(model)
    B = st.shape[1]
    w = f(weights) if weights is not None else None
    hist = np.zeros((steps, 9, B)); status = np.full(B, -99, dtype=np.int32); iters = np.full(B, -99, dtype=np.int32)
    sst = np.zeros((steps, B), dtype=np.int32); sit = np.zeros((steps, B), dtype=np.int32)
    rc = twin.mpc_twin_rollout(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(st), vp(cf), vp(yl), vp(yh), vp(w),
                               vp(md), C.c_int(1 if warm_start else 0), C.byref(opts), vp(hist), vp(status), vp(iters), vp(sst), vp(sit))
    assert rc == 0
    return {"hist": hist, "state": st, "status": status, "iters": iters, "step_status": sst, "step_iters": sit}


def oracle_model_loops(cfgname, sc, model, cars, steps):
    """The oracle's own cold closed loop of the selected cars, each with its own OrcConfig -> {car: (o9 [steps, 9], status [steps])};
    a loop ends at the first solve that does not converge (the later rows stay NaN / -1)."""
    res = {}
    for i in cars:
        over = {name: float(model[q, i]) for q, name in enumerate(MODEL_FIELDS)}
        cfg = O.load_config(cfgname, **over)
        cfg.yaw_low, cfg.yaw_high = float(sc["yaw_lo"][i]), float(sc["yaw_hi"][i])
        o = np.full((steps, 9), np.nan); s = np.full(steps, -1, dtype=np.int32)
        cur = list(sc["state"][:, i])
        for k in range(steps):
            stt, o9, _, _, _ = O.mpc_solve(cfg, cur, sc["coeffs"][:, i])
            o[k] = o9; s[k] = stt
            if stt != 0:
                break
            cur = list(o9[:6])
        res[int(i)] = (o, s)
    return res


def assert_loops_follow_oracle(hist, step_status, loops, what=""):
    """Every solve of the oracle's loops: its status, and where it converges delta0, a0 and the step-1 state within the tolerances."""
    worst = [0.0, 0.0, 0.0]
    n = 0
    for i, (o, s) in loops.items():
        for k in range(len(s)):
            if s[k] < 0:
                break
            assert step_status[k, i] == s[k], (what, i, k, int(step_status[k, i]), int(s[k]))
            if s[k] != 0:
                break
            n += 1
            worst[0] = max(worst[0], abs(hist[k, 6, i] - o[k, 6])); worst[1] = max(worst[1], abs(hist[k, 7, i] - o[k, 7]))
            worst[2] = max(worst[2], float(np.abs(hist[k, :6, i] - o[k, :6]).max()))
    print("%s vs the oracle's loops: %d solves of %d cars, max |d steer| %.3g rad, |d accel| %.3g, |d state| %.3g" %
          (what, n, len(loops), worst[0], worst[1], worst[2]))
    assert n > 0 and worst[0] <= TOL_STEER and worst[1] <= TOL_ACCEL and worst[2] <= TOL_TRAJ, (what, worst)


def steering_outside(params_N, warm, max_steering):
    """columns of a warm buffer that hold a |delta_k| above max_steering_i (1 + 1e-8): the relaxed box of warm_point()"""
    d = np.abs(warm.reshape(params_N - 1, WARM_REC, -1)[:, 6, :])
    return (d > (max_steering * (1.0 + 1e-8))[None, :]).any(0)
