"""Helpers of the tests of track driving with per-car model values (test infrastructure): the CPU build's calls with a model array
(tests/drive_twin through tests/drive_helpers.py), the plant as a composition of the oracle's Vehicle::move with every car's own Lf and max_steering, and the
oracle's telemetry handler with a per-car Config on recorded steps.  Shared by tests/test_drive_model.py and
tests/test_drive_model_gpu.py; tests/drive_helpers.py has everything that does not depend on the model array."""
import numpy as np

import drive_helpers as D
import oracle_lib as O
from drive_helpers import REC_CMD, REC_K, REC_STATUS, TOL_THROTTLE, fast_params, oracle_plant, to_device, window_points      # noqa: F401  (re-exported)
from helpers import TOL_STEER
from run_model_helpers import car_config


def twin_plant_model(twin, params, car, cmd, model, sub_old, sub_new, h):
    return D.twin_plant_call(twin, params, car, cmd, D.plant_opts(params, sub_old, sub_new, h), model=model)[0]


def oracle_plant_model(cfgname, car, cmd, model, sub_old, sub_new, h):
    """drive_helpers.oracle_plant car by car, each with its own Config (Lf) and the reply scaled by its own max_steering"""
    out = np.array(car, dtype=np.float64, copy=True)
    for i in range(out.shape[1]):
        out[:, i:i + 1] = oracle_plant(car_config(cfgname, model, i), out[:, i:i + 1], cmd[:, i:i + 1], float(model[2, i]), sub_old, sub_new, h)
    return out


def twin_handler_model(twin, params, waypoints, car, k, model, opts, warm_opts, weights=None, warm=None, warm_status=None, want_warm=False):
    """One handler call of the CPU build on cars [6, B] with the windows that start at k and the columns of model -> cmd, status,
    iters, cte_epsi, warm."""
    return D.twin_handler_call(twin, params, waypoints, car, k, opts, warm_opts, model=model, weights=weights, warm=warm, warm_status=warm_status,
                               want_warm=want_warm)


def twin_drive_model(twin, params, waypoints, car, model, steps, opts, warm_opts, weights=None):
    """mpc_drive_twin with the arguments of mpc_drive_batch_host_model -> car, summary, hist [steps, 13, B], status, iters."""
    return D.twin_drive_call(twin, params, waypoints, car, steps, opts, warm_opts, model=model, weights=weights)


def oracle_check_steps_model(cfgname, over, model, waypoints, hist, extra):
    """On every recorded (car, window), the oracle's telemetry handler with the car's own Config: the same status, the steer within
    TOL_STEER taken in radians of the car's own max_steering, the throttle within TOL_THROTTLE.  No (car, step) pair is left out.
    -> (max |d steer| [rad], max |d throttle|, pairs compared)."""
    steps, _, B = hist.shape
    d_steer = d_thr = 0.0
    pairs = 0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in range(B):
            cfg = car_config(cfgname, model, i, **over)          # (a fresh one per call: run() mutates the yaw bounds of its Config)
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], extra)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            assert st == 0, (t, i, st)                           # the stated population: every solve ends SUCCESS in the oracle
            d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * float(model[2, i]))
            d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
            pairs += 1
    assert pairs == steps * B
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr, pairs


# ---- the device side (tests/test_drive_model_gpu.py) ------------------------------------------------------------------------------
def device_drive(pkg, params, waypoints, car, model, steps, dev, host=False, fused=False, plain=False, **kw):
    """drive_helpers.device_drive on the _model entry points (plain: the entry points without _model, and no model argument; model
    None otherwise: model = NULL)"""
    return D.device_drive(pkg, params, waypoints, car, steps, dev, model=model, form="host" if host else ("fused" if fused else "device"),
                          entry="" if plain else "model", **kw)


def containment_case(pkg, params, waypoints):
    """80 cars with the columns draw_rows(seed 9), clean and dirty -> car, model, dirty car, dirty model, the cars that must end
    INFEASIBLE at every step (an unusable column: NaN, dt = 0; a car at twice its own top speed), all cars that carry a status."""
    from model_helpers import draw_rows
    car = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    model = draw_rows(params, 80, seed=9)
    d_car, d_model = car.copy(), model.copy()
    d_model[2, 3] = np.nan; d_model[0, 21] = 0.0
    d_model[5, 40] = 0.5 * car[3, 40] * 1609.34 / 3600.0          # its own top speed: half of what it is driving
    d_car[0, 5] = np.nan; d_car[0, 70] += 1e6
    return car, model, d_car, d_model, [3, 21, 40], [3, 21, 40, 5, 70]


def child_runs(pkg, params, waypoints):
    """the clean and the dirty batch of containment_case, for drive_helpers.run_in_child"""
    car, model, d_car, d_model, _, _ = containment_case(pkg, params, waypoints)
    return [("clean", car, dict(entry="model", model=model)), ("dirty", d_car, dict(entry="model", model=d_model))]
