"""Helpers of the tests of track driving with a per-car horizon (test infrastructure): the CPU build's calls with a horizon array
(tests/drive_twin through tests/drive_helpers.py), the oracle's telemetry handler with N = horizon[i] on recorded steps, the unusable horizons, and the device
side through the raw ABI.  Shared by tests/test_drive_horizon.py and tests/test_drive_horizon_gpu.py; tests/drive_helpers.py,
tests/drive_model_helpers.py and tests/drive_latency_helpers.py have everything that does not depend on the horizon array."""
import functools

import numpy as np

import drive_helpers as D
import oracle_lib as O
from drive_helpers import HZ_PAD, KEYS, REC_CMD, REC_K, REC_STATUS, TOL_THROTTLE, fast_params, same, window_points      # noqa: F401  (re-exported)
from drive_latency_helpers import draw_latency, handle_comp, uniform_latency      # noqa: F401  (re-exported)
from helpers import TOL_STEER
from horizon_helpers import LOOP_HORIZONS

INFEASIBLE = 3

def _hz(horizon):
    return np.ascontiguousarray(horizon, dtype=np.int32)


def mixed_horizons(B, choices=LOOP_HORIZONS):
    """choices[i % len(choices)]"""
    return _hz([choices[i % len(choices)] for i in range(B)])


def default_latency(params, opts, B):
    """the columns that say what the call's own scalars say (twin_drive_horizon always passes a latency array)"""
    return uniform_latency(B, handle_comp(params, opts.extra_latency), opts.sub_old, opts.sub_new)


def twin_drive_horizon(twin, params, waypoints, car, horizon, steps, opts, warm_opts, model=None, latency=None, weights=None):
    """mpc_drive_twin with the arguments of mpc_drive_batch_host_horizon -> car, summary, hist [steps, 13, B], status, iters.
    latency None: the columns of the call's own scalars."""
    latency = latency if latency is not None else default_latency(params, opts, np.shape(car)[1])
    return D.twin_drive_call(twin, params, waypoints, car, steps, opts, warm_opts, model=model, horizon=_hz(horizon), latency=latency, weights=weights)


def twin_handler_horizon(twin, params, waypoints, car, comp, k, horizon, opts, warm_opts, model=None, weights=None, warm=None, warm_status=None,
                         want_warm=False):
    """One handler call of the CPU build on cars [6, B] with the windows that start at k, compensating comp [B], horizon [B] -> cmd,
    status, iters, cte_epsi, warm (the rows of params.N)."""
    return D.twin_handler_call(twin, params, waypoints, car, k, opts, warm_opts, comp=comp, model=model, horizon=_hz(horizon), weights=weights, warm=warm,
                               warm_status=warm_status, want_warm=want_warm, keep_warm=True)


def oracle_check_steps_horizon(cfgname, params, horizon, waypoints, hist, extra=0.0):
    """On every recorded (car, window), the oracle's telemetry handler on a config loaded with N = horizon[i]: the same status, the steer
    within TOL_STEER / max_steering and the throttle within TOL_THROTTLE (the bounds of drive_helpers.oracle_check_steps).  No (car,
    step) pair is left out.  -> (max |d steer| [rad], max |d throttle|, pairs compared)."""
    steps, _, B = hist.shape
    d_steer = d_thr = 0.0
    pairs = 0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in range(B):
            cfg = O.load_config(cfgname, N=int(horizon[i]))          # (a fresh one per call: run() mutates it)
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], extra)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            assert st == 0, (t, i, st)                                # the stated inputs: every solve ends SUCCESS
            d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * params.max_steering)
            d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
            pairs += 1
    assert pairs == steps * B
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr, pairs


def unusable(horizon, cars, N):
    """The four unusable horizons of the issue -- 2, 0, -1, N + 1 -- in the cars `cars` (4 of them) of a copy."""
    d = _hz(horizon).copy()
    d[list(cars)] = [2, 0, -1, N + 1]
    return d


def check_unusable(res, clean, bad, steps):
    """those cars INFEASIBLE at every step, summary row 7 = steps, no not-a-number; every other car bitwise the clean batch"""
    assert (res["hist"][:, REC_STATUS][:, bad] == INFEASIBLE).all() and (res["status"][bad] == INFEASIBLE).all()
    assert (res["summary"][7, bad] == steps).all()
    for k in ("car", "summary", "hist"):
        assert np.isfinite(res[k][..., bad]).all(), k
    good = np.setdiff1d(np.arange(res["status"].shape[0]), bad)
    same(res, clean, cars=good)


# ---- the device side (tests/test_drive_horizon_gpu.py) ----------------------------------------------------------------------------
device_drive = functools.partial(D.device_drive, entry="horizon")      # (entry="latency": the _latency entry points, no horizon argument)


BAD_HORIZONS = [3, 21, 40, 55]         # the cars of containment_case with an unusable horizon (2, 0, -1, N + 1)
BAD_CARS = [5, 70]                     # ... and those no caller should send: x = NaN, 1e6 m off the track


def containment_case(pkg, params, waypoints):
    """80 cars with the horizons LOOP_HORIZONS[i % 5], clean and dirty -> car, horizon, dirty car, dirty horizon."""
    car = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    hz = mixed_horizons(80)
    d_car, d_hz = car.copy(), unusable(hz, BAD_HORIZONS, params.N)
    d_car[0, 5] = np.nan; d_car[0, 70] += 1e6
    return car, hz, d_car, d_hz


def child_runs(pkg, params, waypoints):
    """the clean and the dirty batch of containment_case, for drive_helpers.run_in_child"""
    car, hz, d_car, d_hz = containment_case(pkg, params, waypoints)
    return [("clean", car, dict(entry="horizon", horizon=hz)), ("dirty", d_car, dict(entry="horizon", horizon=d_hz))]
