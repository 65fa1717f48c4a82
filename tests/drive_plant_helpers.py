"""Helpers of the tests of track driving with per-car plant values (test infrastructure): the TEST-ONLY CPU build of the plant loop
(tests/drive_plant_twin), the drawn columns, the substep of include/mpc_amd_drive.h ("per-car plant values") written once more from
its text in a number format of the caller's choice, and the raw-ABI call of the three _plant forms.  Shared by
tests/test_drive_plant.py and tests/test_drive_plant_gpu.py; tests/drive_helpers.py, tests/drive_model_helpers.py and
tests/drive_latency_helpers.py have everything that does not depend on the plant array."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

from drive_helpers import ISENTINEL, NSUM, REC, SENTINEL, _f, track_of
from drive_latency_helpers import KEYS, same  # noqa: F401  (re-exported: the tests compare with them)
from drive_model_helpers import fast_params, to_device
from helpers import ROOT, vp

LF, GAIN, BIAS, ACCEL, DRAG, DRIFT = range(6)
SUCCESS, INFEASIBLE, ACCEPTABLE = 0, 3, 6
_twin = None


def load_drive_plant_twin():
    global _twin
    if _twin is None:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's own comes first, as in _abi.library)
        except ImportError:
            pass
        d = os.path.join(ROOT, "tests", "drive_plant_twin")
        subprocess.check_call(["make", "-s", "-C", d])
        _twin = C.CDLL(os.path.join(d, "libdrive_plant_twin.so"))
    return _twin


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
    car, cmd, model, plant = _f(car).copy(), _f(cmd), _f(model), _f(plant)
    B = car.shape[1]
    assert model.shape == (6, B) and plant.shape == (6, B)
    ok = np.zeros(B, dtype=np.int32)
    rc = twin.mpc_drive_plant_twin_plant(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(cmd), vp(model), vp(plant), C.c_int(sub_old),
                                         C.c_int(sub_new), C.c_double(h), vp(ok))
    assert rc == 0, rc
    return car, ok


def twin_drive_plant(twin, params, waypoints, car, model, latency, plant, steps, opts, warm_opts, weights=None):
    """mpc_drive_plant_twin with the arguments of mpc_drive_batch_host_plant (no horizon) -> car, summary, hist [steps, 13, B], status,
    iters, and handler_status [steps, B]: the handler's own status of every step."""
    tx, ty = track_of(waypoints)
    car, model, latency, plant = _f(car).copy(), _f(model), _f(latency), _f(plant)
    B = car.shape[1]
    assert model.shape == (6, B) and latency.shape == (3, B) and plant.shape == (6, B)
    summary = np.full((NSUM, B), SENTINEL); hist = np.full((steps, REC, B), SENTINEL)
    status = np.full(B, ISENTINEL, dtype=np.int32); iters = np.full(B, ISENTINEL, dtype=np.int32)
    hs = np.full((steps, B), ISENTINEL, dtype=np.int32)
    rc = twin.mpc_drive_plant_twin(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(car), vp(tx), vp(ty), C.c_int(len(tx)),
                                   vp(_f(weights)), vp(model), vp(latency), vp(plant), C.byref(opts), C.byref(warm_opts), vp(summary), vp(hist),
                                   vp(status), vp(iters), vp(hs))
    assert rc == 0, rc
    return {"car": car, "summary": summary, "hist": hist, "status": status, "iters": iters, "handler_status": hs}


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
CHILD_TIMEOUT_S = 120
FORMS = {"device": "mpc_drive_batch_device", "fused": "mpc_drive_batch_device_fused", "host": "mpc_drive_batch_host"}


def device_drive(pkg, params, waypoints, car, steps, dev, model=None, horizon=None, latency=None, plant=None, form="device", entry="plant", warm=0,
                 weights=None, hist=True, pad=3, opts_over=None, mpc=None):
    """A drive entry point through the raw ABI with ld = B + pad.  entry: "plant" (model, horizon, latency and plant may each be None:
    NULL) or "horizon" (no plant argument).  Inputs hold NaN (horizon: 0) from column B on, outputs the sentinels everywhere before
    the call.  -> the arrays cut to B, after checking that nothing behind column B was written; and the handle's mpc_drive_info."""
    import torch
    lib = pkg.library()
    B = car.shape[1]
    ld = B + pad
    tx, ty = track_of(waypoints)
    opts = pkg.drive_opts_default(params, warm_start=warm, **(opts_over or {}))

    def wide(a, fill=np.nan):
        if a is None:
            return None
        w = np.full((a.shape[0], ld), fill); w[:, :B] = a
        return w
    h_car, h_w, h_m, h_l, h_p = wide(car), wide(weights), wide(model), wide(latency), wide(plant)
    h_hz = None
    if horizon is not None:
        h_hz = np.zeros(ld, dtype=np.int32); h_hz[:B] = horizon
    h_sum = np.full((NSUM, ld), SENTINEL); h_hist = np.full((steps, REC, ld), SENTINEL) if hist else None
    h_st = np.full(ld, ISENTINEL, dtype=np.int32); h_it = np.full(ld, ISENTINEL, dtype=np.int32)
    host = form == "host"
    call = getattr(lib, FORMS[form] + "_" + entry)
    own = mpc is None
    if own:
        mpc = pkg.BatchedMPC(params, max(B, 1), device=0)
    try:
        if host:
            p = lambda a: a.ctypes.data if a is not None else None
            ex = (p(h_m), p(h_hz), p(h_l)) + ((p(h_p),) if entry == "plant" else ())
            rc = call(mpc._h, B, ld, steps, p(h_car), p(tx), p(ty), len(tx), p(h_w), *ex, C.byref(opts), None, p(h_sum), p(h_hist), p(h_st), p(h_it))
            assert rc == 0, lib.mpc_last_error()
            got = {"car": h_car, "summary": h_sum, "hist": h_hist, "status": h_st, "iters": h_it}
        else:
            dd = lambda a, dt=np.float64: to_device(a, dev, dt) if a is not None else None
            d = {"car": dd(h_car), "summary": dd(h_sum), "hist": dd(h_hist), "status": dd(h_st, np.int32), "iters": dd(h_it, np.int32)}
            d_tx, d_ty, d_w, d_m, d_l, d_p, d_hz = dd(tx), dd(ty), dd(h_w), dd(h_m), dd(h_l), dd(h_p), dd(h_hz, np.int32)
            p = lambda t: t.data_ptr() if t is not None else None
            ex = (p(d_m), p(d_hz), p(d_l)) + ((p(d_p),) if entry == "plant" else ())
            rc = call(mpc._h, B, ld, steps, p(d["car"]), p(d_tx), p(d_ty), len(tx), p(d_w), *ex, C.byref(opts), None, p(d["summary"]), p(d["hist"]),
                      p(d["status"]), p(d["iters"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert rc == 0, lib.mpc_last_error()
            torch.cuda.synchronize()
            got = {k: (v.cpu().numpy() if v is not None else None) for k, v in d.items()}
        info = mpc.drive_info()
    finally:
        if own:
            mpc.close()
    assert np.isnan(got["car"][:, B:]).all() and (got["summary"][:, B:] == SENTINEL).all() and (got["status"][B:] == ISENTINEL).all() and (got["iters"][B:] == ISENTINEL).all()
    if hist:
        assert (got["hist"][:, :, B:] == SENTINEL).all()
    out = {k: (v[..., :B].copy() if v is not None else None) for k, v in got.items()}
    assert (out["summary"] != SENTINEL).all() and (out["status"] != ISENTINEL).all() and (out["iters"] != ISENTINEL).all()
    out["info"] = info
    return out


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


def child_main(path):
    """Runs in the child: the clean and the dirty batch of unusable_case on the device, cold and warm, results into an .npz."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    import torch
    pkg = G.load_package()
    spec = json.load(open(path + ".json"))
    gd = os.path.join(ROOT, "tests", "golden")
    params = fast_params(pkg, gd, wave_max_batch=spec["wave_max_batch"])
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    car, plant, dirty, _ = unusable_case(pkg, params, wp)
    dev = torch.device("cuda:0")
    out = {}
    for warm in (0, 1):
        for tag, pl in (("clean", plant), ("dirty", dirty)):
            r = device_drive(pkg, params, wp, car, 4, dev, plant=pl, warm=warm, form="fused" if spec["fused"] else "device")
            for k in KEYS:
                out["%d/%s/%s" % (warm, tag, k)] = r[k]
            out["%d/%s/info" % (warm, tag)] = np.array([r["info"]["fused_launches"], r["info"]["stepwise_loops"]])
    np.savez(path, **out)


def run_unusable_in_child(wave_max_batch, fused, timeout=CHILD_TIMEOUT_S):
    """-> {(warm, "clean" | "dirty"): the arrays of device_drive}; a child that does not end within `timeout` seconds fails the caller
    (subprocess.TimeoutExpired) after it has been killed"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "unusable.npz")
        json.dump({"wave_max_batch": int(wave_max_batch), "fused": bool(fused)}, open(path + ".json", "w"))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=timeout, env=env)
        assert p.returncode == 0, p.stderr[-4000:]
        z = np.load(path)
        res = {}
        for key in z.files:
            warm, tag, k = key.split("/")
            res.setdefault((int(warm), tag), {})[k] = z[key]
        for r in res.values():
            r["info"] = {"fused_launches": int(r["info"][0]), "stepwise_loops": int(r["info"][1])}
    return res


if __name__ == "__main__":
    child_main(sys.argv[1])
