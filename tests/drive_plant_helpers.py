"""Helpers of the tests of track driving with per-car plant values (test infrastructure): the CPU build's calls with a plant array
(tests/drive_twin through tests/drive_helpers.py), the drawn columns, the substep of include/mpc_amd_drive.h ("per-car plant values") written once more from
its text in a number format of the caller's choice, and the raw-ABI call of the three _plant forms.  Shared by
tests/test_drive_plant.py and tests/test_drive_plant_gpu.py; tests/drive_helpers.py, tests/drive_model_helpers.py and
tests/drive_latency_helpers.py have everything that does not depend on the plant array."""
import functools

import numpy as np

import drive_helpers as D
from drive_helpers import KEYS, same  # noqa: F401  (re-exported: the tests compare with them)

LF, GAIN, BIAS, ACCEL, DRAG, DRIFT = range(6)
SUCCESS, INFEASIBLE, ACCEPTABLE = 0, 3, 6

def draw_plant(B, seed=31):
    """The stated population: Lf 1.5 .. 4.5, g 0.7 .. 1.3, b +-0.05, a 3 .. 9, d 30 .. 80, w +-1, uniform, in row order."""
    g = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([g.uniform(1.5, 4.5, B), g.uniform(0.7, 1.3, B), g.uniform(-0.05, 0.05, B), g.uniform(3.0, 9.0, B),
                                          g.uniform(30.0, 80.0, B), g.uniform(-1.0, 1.0, B)]))


def uniform_plant(B, col):
    return np.ascontiguousarray(np.repeat(np.asarray(col, dtype=np.float64)[:, None], B, axis=1))


def reference_plant(car, cmd, max_steering, plant, sub_old, sub_new, h, dtype=np.longdouble):
    """The plant of the header's text in `dtype`, every operation rounded on its own (no fused multiply-add): sub_old substeps, the
    reply takes effect as (cmd_steer * max_steering, cmd_throttle) unless it is not finite, sub_new substeps.  -> car [6, B] in dtype."""
    c = np.array(car, dtype=dtype, copy=True)
    lf, g, b, a, d, w = (np.asarray(r, dtype=dtype) for r in plant)
    h = dtype(h)

    def substep():
        v = c[3] * dtype(1609.34) / dtype(3600)
        steer = -(c[4] * g + b)
        accel = (c[5] - v / d) * a
        dist = v * h
        sn, cs = np.sin(c[2]), np.cos(c[2])
        x = c[0] + dist * cs
        x = x - (w * h) * sn
        y = c[1] + dist * sn
        y = y + (w * h) * cs
        psi = c[2] + steer * dist / lf
        speed = (v + accel * h) * dtype(3600) / dtype(1609.34)
        c[0], c[1], c[2], c[3] = x, y, psi, speed
    for _ in range(sub_old):
        substep()
    cmd = np.asarray(cmd, dtype=np.float64)
    ok = np.isfinite(cmd[0]) & np.isfinite(cmd[1])
    c[4, ok] = (cmd[0, ok] * max_steering).astype(dtype)      # (the product is the build's own: one double multiplication)
    c[5, ok] = cmd[1, ok].astype(dtype)
    for _ in range(sub_new):
        substep()
    return c


def twin_plant(twin, params, car, cmd, model, plant, sub_old, sub_new, h):
    """-> the moved cars [6, B] and ok [B] (whether each column could be used)"""
    return D.twin_plant_call(twin, params, car, cmd, D.plant_opts(params, sub_old, sub_new, h), model=model, plant=plant)


def twin_drive_plant(twin, params, waypoints, car, model, latency, plant, steps, opts, warm_opts, weights=None):
    """mpc_drive_twin with the arguments of mpc_drive_batch_host_plant (no horizon) -> car, summary, hist [steps, 13, B], status,
    iters, and handler_status [steps, B]: the handler's own status of every step."""
    return D.twin_drive_call(twin, params, waypoints, car, steps, opts, warm_opts, model=model, latency=latency, plant=plant, weights=weights)


def unusable_columns(default_col):
    """Every unusable column the header names, as (label, column): not-a-number and +infinity in each of the six rows, Lf_p = 0 and -1,
    d = 0 -- 15 of them, each the default column with one value replaced."""
    out = []
    for r in range(6):
        for v in (np.nan, np.inf):
            c = np.array(default_col, dtype=np.float64); c[r] = v
            out.append(("row %d = %s" % (r, v), c))
    for r, v in ((LF, 0.0), (LF, -1.0), (DRAG, 0.0)):
        c = np.array(default_col, dtype=np.float64); c[r] = v
        out.append(("row %d = %s" % (r, v), c))
    return out


def expected_status(handler_status):
    """the status rule of an unusable column: SUCCESS and ACCEPTABLE become INFEASIBLE, every other status stays"""
    hs = np.asarray(handler_status)
    return np.where((hs == SUCCESS) | (hs == ACCEPTABLE), INFEASIBLE, hs)


# ---- the device side (tests/test_drive_plant_gpu.py) --------------------------------------------------------------------------------
device_drive = functools.partial(D.device_drive, entry="plant")        # (entry="horizon": the _horizon entry points, no plant argument)


BAD_AT = 3          # the first car of unusable_case with an unusable column; the others follow at a stride of 4


def unusable_case(pkg, params, waypoints):
    """80 cars with the columns draw_plant(80, seed 32), clean and dirty: the 15 unusable columns in cars 3, 7, 11 ... 59 ->
    car, plant, dirty plant, the dirty cars."""
    car = pkg.scenarios.track_starts(80, params, waypoints, seed=8)
    plant = draw_plant(80, seed=32)
    dirty = plant.copy()
    cols = unusable_columns(pkg.drive_plant_default(params))
    bad = [BAD_AT + 4 * j for j in range(len(cols))]
    for i, (_, c) in zip(bad, cols):
        dirty[:, i] = c
    return car, plant, dirty, bad


def child_runs(pkg, params, waypoints):
    """the clean and the dirty batch of unusable_case, for drive_helpers.run_in_child"""
    car, plant, dirty, _ = unusable_case(pkg, params, waypoints)
    return [("clean", car, dict(entry="plant", plant=plant)), ("dirty", car, dict(entry="plant", plant=dirty))]
