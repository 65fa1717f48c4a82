"""Helpers of the fused-rollout tests (test infrastructure): the TEST-ONLY CPU build of one car's whole loop (mpc_twin_rollout of
tests/host_twin)."""
import ctypes as C

import numpy as np

from helpers import load_twin, vp

load_rollout_twin = load_twin


def twin_rollout(twin, params, sc, steps, opts, warm_start, weights=None):
    """Every car's closed loop, car by car, through mpc::RolloutCar (the arguments of mpc_rollout_batch_device_fused) ->
    hist [steps, 9, B], the final state [6, B], worst status and summed iterations [B], status and iterations of every solve [steps, B]."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh = f(sc["state"]).copy(), f(sc["coeffs"]), f(sc["yaw_lo"]), f(sc["yaw_hi"])
    B = st.shape[1]
    w = f(weights) if weights is not None else None
    hist = np.zeros((steps, 9, B)); status = np.full(B, -99, dtype=np.int32); iters = np.full(B, -99, dtype=np.int32)
    sst = np.zeros((steps, B), dtype=np.int32); sit = np.zeros((steps, B), dtype=np.int32)
    rc = twin.mpc_twin_rollout(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(st), vp(cf), vp(yl), vp(yh), vp(w),
                               None, C.c_int(1 if warm_start else 0), C.byref(opts), vp(hist), vp(status), vp(iters), vp(sst), vp(sit))
    assert rc == 0
    return {"hist": hist, "state": st, "status": status, "iters": iters, "step_status": sst, "step_iters": sit}
