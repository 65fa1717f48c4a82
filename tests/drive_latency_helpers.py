"""Helpers of the tests of track driving with per-car latency (test infrastructure): the CPU build's calls with a latency array
(tests/drive_twin through tests/drive_helpers.py), the drawn columns, the plant as a composition of the oracle's Vehicle::move with every car's own substep
counts, and the oracle's telemetry handler with a per-car Config (latency, lookahead) on recorded steps.  Shared by
tests/test_drive_latency.py and tests/test_drive_latency_gpu.py; tests/drive_helpers.py and tests/drive_model_helpers.py have
everything that does not depend on the latency array."""
import functools

import numpy as np

import drive_helpers as D
import oracle_lib as O
from drive_helpers import KEYS, REC_CMD, REC_K, REC_STATUS, TOL_THROTTLE, oracle_plant, same, window_points      # noqa: F401  (re-exported)
from helpers import TOL_STEER

COMP, SUB_OLD, SUB_NEW = 0, 1, 2

def draw_latency(B, seed=21):
    """The stated population, drawn in this order with default_rng(seed): comp uniform in [0, 0.25] s, then about a quarter of the cars
    (uniform < 0.25) set to exactly 0; sub_old an integer in 0..25; sub_new an integer in 1..12.  Final ranges: the stated ones, not narrowed; final seed: 21.  On
    the 16 cars x 8 messages of tests/test_drive_latency.py (config-fast and config-stable, cold and warm) the oracle alone ends every
    recorded solve SUCCESS with them, so no (car, step) pair is left out of a comparison."""
    g = np.random.default_rng(seed)
    comp = g.uniform(0.0, 0.25, B)
    comp[g.uniform(0.0, 1.0, B) < 0.25] = 0.0
    return np.ascontiguousarray(np.stack([comp, g.integers(0, 26, B).astype(np.float64), g.integers(1, 13, B).astype(np.float64)]))


def uniform_latency(B, comp, sub_old, sub_new):
    return np.ascontiguousarray(np.repeat(np.array([[float(comp)], [float(sub_old)], [float(sub_new)]]), B, axis=1))


def handle_comp(params, extra=0.0):
    """what a handle's own rule compensates for: lookahead + extra_latency, or 0 on a handle with latency_ms = 0"""
    return params.lookahead + extra if params.latency_ms != 0 else 0.0


def twin_plant_latency(twin, params, car, cmd, model, latency, opts):
    return D.twin_plant_call(twin, params, car, cmd, opts, model=model, latency=latency)[0]


def oracle_plant_latency(cfgname, car, cmd, max_steering, latency, h):
    """drive_helpers.oracle_plant car by car, each with its own substep counts"""
    out = np.array(car, dtype=np.float64, copy=True)
    cfg = O.load_config(cfgname)
    for i in range(out.shape[1]):
        out[:, i:i + 1] = oracle_plant(cfg, out[:, i:i + 1], cmd[:, i:i + 1], max_steering, int(latency[SUB_OLD, i]), int(latency[SUB_NEW, i]), h)
    return out


def twin_handler_latency(twin, params, waypoints, car, comp, k, model, opts, warm_opts, weights=None, warm=None, warm_status=None, want_warm=False):
    """One handler call of the CPU build on cars [6, B] with the windows that start at k, compensating comp [B] -> cmd, status, iters,
    cte_epsi, warm."""
    return D.twin_handler_call(twin, params, waypoints, car, k, opts, warm_opts, comp=comp, model=model, weights=weights, warm=warm,
                               warm_status=warm_status, want_warm=want_warm)


def twin_drive_latency(twin, params, waypoints, car, model, latency, steps, opts, warm_opts, weights=None):
    """mpc_drive_twin with the arguments of mpc_drive_batch_host_latency -> car, summary, hist [steps, 13, B], status, iters."""
    return D.twin_drive_call(twin, params, waypoints, car, steps, opts, warm_opts, model=model, latency=latency, weights=weights)


def oracle_check_steps_latency(cfgname, over, params, latency, waypoints, hist):
    """On every recorded (car, window), the oracle's telemetry handler with the car's own Config -- latency = 1 if comp > 0 else 0,
    lookahead = comp -- and extra = 0: the same status, the steer within TOL_STEER (radians), the throttle within TOL_THROTTLE.  No
    (car, step) pair is left out.  -> (max |d steer| [rad], max |d throttle|, pairs compared)."""
    steps, _, B = hist.shape
    d_steer = d_thr = 0.0
    pairs = 0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in range(B):
            comp = float(latency[COMP, i])
            cfg = O.load_config(cfgname, **dict(over, latency=1 if comp > 0 else 0, lookahead=comp))     # (a fresh one per call: run() mutates it)
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], 0.0)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            assert st == 0, (t, i, st)                           # the stated population: every solve ends SUCCESS in the oracle
            d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * params.max_steering)
            d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
            pairs += 1
    assert pairs == steps * B
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr, pairs


def unusable(latency, cars):
    """The four unusable columns of the issue in the cars `cars` (4 of them) of a copy: NaN, comp = -1, sub_old = 2.5,
    sub_old + sub_new = 1001."""
    d = np.array(latency, dtype=np.float64, copy=True)
    a, b, c, e = cars
    d[COMP, a] = np.nan
    d[COMP, b] = -1.0
    d[SUB_OLD, c] = 2.5
    d[SUB_OLD, e] = 1001.0 - d[SUB_NEW, e]
    return d


# ---- the device side (tests/test_drive_latency_gpu.py) ----------------------------------------------------------------------------
device_drive = functools.partial(D.device_drive, entry="latency")      # (entry="model": the _model entry points, no latency argument)


BAD_COLUMNS = [3, 21, 40, 55]          # the cars of containment_case with an unusable column
BAD_CARS = [5, 70]                     # ... and those no caller should send: x = NaN, 1e6 m off the track


def containment_case(pkg, params, waypoints):
    """80 cars with the columns draw_latency(80, seed 22), clean and dirty -> car, latency, dirty car, dirty latency."""
    car = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    latency = draw_latency(80, seed=22)
    d_car, d_lat = car.copy(), unusable(latency, BAD_COLUMNS)
    d_car[0, 5] = np.nan; d_car[0, 70] += 1e6
    return car, latency, d_car, d_lat


def child_runs(pkg, params, waypoints):
    """the clean and the dirty batch of containment_case, for drive_helpers.run_in_child"""
    car, lat, d_car, d_lat = containment_case(pkg, params, waypoints)
    return [("clean", car, dict(entry="latency", latency=lat)), ("dirty", d_car, dict(entry="latency", latency=d_lat))]
