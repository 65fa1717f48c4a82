"""Helpers of the track-driving tests (test infrastructure): the TEST-ONLY CPU build of the drive loop (tests/drive_twin: one library
for every form, and one call of each of its functions here), numpy's statement of the summary rows, the plant as a composition of the
oracle's Vehicle::move, the oracle's telemetry handler on recorded steps -- the comparison is solve by solve, so loop amplification
cannot enter --, and the device side of every form: the raw-ABI call of a drive entry point and the child process that runs a batch
with cars no caller should send.  Shared by the tests/test_drive*.py; the drive_*_helpers.py modules hold what depends on one per-car
array."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import oracle_lib as O
from helpers import ROOT, TOL_STEER, vp

NSUM, REC = 8, 13
REC_CMD, REC_CTE, REC_EPSI, REC_STATUS, REC_ITERS, REC_K = 6, 8, 9, 10, 11, 12
TOL_THROTTLE = 1e-5        # the bound tests/test_run_warm_gpu.py uses for the handler's throttle
SENTINEL, ISENTINEL = -7777.25, -12345

_twin = None


def load_drive_twin():
    global _twin
    if _twin is None:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's own comes first, as in _abi.library)
        except ImportError:
            pass
        d = os.path.join(ROOT, "tests", "drive_twin")
        subprocess.check_call(["make", "-s", "-C", d])
        _twin = C.CDLL(os.path.join(d, "libdrive_twin.so"))
    return _twin


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64) if a is not None else None


def track_of(waypoints):
    wp = np.asarray(waypoints, dtype=np.float64)
    return np.ascontiguousarray(wp[:, 0]), np.ascontiguousarray(wp[:, 1])


def twin_window(twin, waypoints, x, y):
    tx, ty = track_of(waypoints)
    x, y = _f(x), _f(y)
    k = np.full(len(x), ISENTINEL, dtype=np.int32)
    assert twin.mpc_drive_twin_window(vp(tx), vp(ty), C.c_int(len(tx)), C.c_int64(len(x)), vp(x), vp(y), vp(k)) == 0
    return k


def window_points(waypoints, k, npts=6):
    """w[k .. k + npts - 1], cyclically -> ptsx, ptsy [npts, B]"""
    wp = np.asarray(waypoints, dtype=np.float64)
    idx = (np.asarray(k, dtype=np.int64)[None, :] + np.arange(npts)[:, None]) % len(wp)
    return np.ascontiguousarray(wp[idx, 0]), np.ascontiguousarray(wp[idx, 1])


def plant_opts(params, sub_old, sub_new, h):
    """the handle's default MpcDriveOpts with these substep counts and this substep length"""
    import __graft_entry__ as G
    return G.load_package().drive_opts_default(params, sub_old=sub_old, sub_new=sub_new, h=h)


def twin_plant_call(twin, params, car, cmd, opts, model=None, latency=None, plant=None):
    """mpc_drive_twin_plant: the cars moved with opts' counts (latency: their own) and substep length; model, latency and plant [., B]
    or None (NULL) -> the moved cars [6, B] and ok [B] (whether each plant column could be used)"""
    car, cmd, model, latency, plant = _f(car).copy(), _f(cmd), _f(model), _f(latency), _f(plant)
    B = car.shape[1]
    assert all(a is None or a.shape == (n, B) for a, n in ((model, 6), (latency, 3), (plant, 6)))
    ok = np.zeros(B, dtype=np.int32)
    rc = twin.mpc_drive_twin_plant(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(cmd), vp(model), vp(latency), vp(plant), C.byref(opts), vp(ok))
    assert rc == 0, rc
    return car, ok


def twin_plant(twin, params, car, cmd, sub_old, sub_new, h):
    return twin_plant_call(twin, params, car, cmd, plant_opts(params, sub_old, sub_new, h))[0]


def oracle_plant(cfg, car, cmd, max_steering, sub_old, sub_new, h):
    """The plant as the issue states it, one car at a time: substeps of the oracle's Vehicle::move (O.vehicle_move) under the handler's
    reading of the car -- v = mph2mps(speed), steer = -steering_angle, accel = (throttle - v / 50) * 6 --, the reply taking effect after
    sub_old of them unless it is not finite."""
    out = np.array(car, dtype=np.float64, copy=True)
    for i in range(out.shape[1]):
        c = out[:, i].copy()

        def sub():
            v = c[3] * 1609.34 / 3600.0
            p = O.vehicle_move(cfg, [c[0], c[1], c[2], v, -c[4], (c[5] - v / 50.0) * 6.0], h)
            c[0], c[1], c[2], c[3] = p[0], p[1], p[2], p[3] * 3600.0 / 1609.34
        for _ in range(sub_old):
            sub()
        if np.isfinite(cmd[0, i]) and np.isfinite(cmd[1, i]):
            c[4], c[5] = cmd[0, i] * max_steering, cmd[1, i]
        for _ in range(sub_new):
            sub()
        out[:, i] = c
    return out


def numpy_plant(car, cmd, params, sub_old, sub_new, h):
    """The plant for a whole batch in numpy (the loop a caller writes without the drive entry points; tools/drive_bench.py): the
    substeps of oracle_plant, vectorised.  -> the next cars [6, B]."""
    def sub(c):
        v = c[3] * 1609.34 / 3600.0
        dist = v * h
        acc = (c[5] - v / 50.0) * 6.0
        return np.stack([c[0] + dist * np.cos(c[2]), c[1] + dist * np.sin(c[2]), c[2] - c[4] * dist / params.Lf, (v + acc * h) * 3600.0 / 1609.34, c[4], c[5]])
    car = np.array(car, dtype=np.float64, copy=True)
    for _ in range(sub_old):
        car = sub(car)
    ok = np.isfinite(cmd[0]) & np.isfinite(cmd[1])
    car[4] = np.where(ok, cmd[0] * params.max_steering, car[4]); car[5] = np.where(ok, cmd[1], car[5])
    for _ in range(sub_new):
        car = sub(car)
    return np.ascontiguousarray(car)


def twin_handler_call(twin, params, waypoints, car, k, opts, warm_opts, comp=None, model=None, horizon=None, weights=None, warm=None, warm_status=None,
                      want_warm=False, keep_warm=False):
    """mpc_drive_twin_handler: one handler call of the CPU build on cars [6, B] with the windows that start at k; comp [B] (None:
    opts.extra_latency), model [6, B] and horizon [B] or None (NULL) -> cmd, status, iters, cte_epsi, warm (the rows of params.N;
    keep_warm: the rows the call does not write keep what `warm` held)."""
    tx, ty = track_of(waypoints)
    car, model, comp = _f(car), _f(model), _f(comp)
    B = car.shape[1]
    k = np.ascontiguousarray(k, dtype=np.int32)
    horizon = np.ascontiguousarray(horizon, dtype=np.int32) if horizon is not None else None
    rows = (params.N - 1) * 22
    cmd = np.zeros((2, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32); ce = np.zeros((2, B))
    wout = None
    if want_warm or warm is not None:
        wout = np.array(warm, dtype=np.float64, copy=True) if (keep_warm and warm is not None) else np.zeros((rows, B))
    warm = _f(warm)
    if warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_drive_twin_handler(C.byref(params), C.c_int64(B), C.c_int64(B), vp(car), vp(comp), vp(k), vp(tx), vp(ty), C.c_int(len(tx)), vp(_f(weights)),
                                     vp(model), vp(horizon), C.byref(opts), vp(warm), vp(warm_status), vp(wout), C.c_int64(B), C.byref(warm_opts), vp(cmd),
                                     vp(status), vp(iters), vp(ce))
    assert rc == 0, rc
    return {"cmd": cmd, "status": status, "iters": iters, "cte_epsi": ce, "warm": wout}


def twin_handler(twin, params, waypoints, car, k, opts, warm_opts, weights=None, warm=None, warm_status=None, want_warm=False):
    return twin_handler_call(twin, params, waypoints, car, k, opts, warm_opts, weights=weights, warm=warm, warm_status=warm_status, want_warm=want_warm)


def twin_drive_call(twin, params, waypoints, car, steps, opts, warm_opts, model=None, horizon=None, latency=None, plant=None, weights=None):
    """mpc_drive_twin with the arguments of mpc_drive_batch_host_plant, each per-car array or None (NULL) -> car, summary,
    hist [steps, 13, B], status, iters, and handler_status [steps, B]: the handler's own status of every step."""
    tx, ty = track_of(waypoints)
    car, model, latency, plant = _f(car).copy(), _f(model), _f(latency), _f(plant)
    B = car.shape[1]
    horizon = np.ascontiguousarray(horizon, dtype=np.int32) if horizon is not None else None
    assert all(a is None or a.shape == (n, B) for a, n in ((model, 6), (latency, 3), (plant, 6))) and (horizon is None or horizon.shape == (B,))
    summary = np.full((NSUM, B), SENTINEL); hist = np.full((steps, REC, B), SENTINEL)
    status = np.full(B, ISENTINEL, dtype=np.int32); iters = np.full(B, ISENTINEL, dtype=np.int32)
    hs = np.full((steps, B), ISENTINEL, dtype=np.int32)
    rc = twin.mpc_drive_twin(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(steps), vp(car), vp(tx), vp(ty), C.c_int(len(tx)), vp(_f(weights)),
                             vp(model), vp(horizon), vp(latency), vp(plant), C.byref(opts), C.byref(warm_opts), vp(summary), vp(hist), vp(status),
                             vp(iters), vp(hs))
    assert rc == 0, rc
    return {"car": car, "summary": summary, "hist": hist, "status": status, "iters": iters, "handler_status": hs}


def twin_drive(twin, params, waypoints, car, steps, opts, warm_opts, weights=None):
    """mpc_drive_twin with the arguments of mpc_drive_batch_host"""
    return twin_drive_call(twin, params, waypoints, car, steps, opts, warm_opts, weights=weights)


def summary_from_hist(hist, n_track, cte_limit):
    """The summary rows recomputed from the records, in step order (a not-a-number never wins a maximum or the minimum)."""
    steps, _, B = hist.shape
    s = np.zeros((NSUM, B))
    s[4] = np.inf; s[6] = -1.0
    for t in range(steps):
        cte, epsi, speed = hist[t, REC_CTE], hist[t, REC_EPSI], hist[t, 3]
        ac, ae = np.abs(cte), np.abs(epsi)
        s[0] = np.where(ac > s[0], ac, s[0]); s[1] = s[1] + cte * cte; s[2] = np.where(ae > s[2], ae, s[2])
        s[3] = s[3] + speed; s[4] = np.where(speed < s[4], speed, s[4])
        if t > 0:
            d = (hist[t, REC_K] - hist[t - 1, REC_K]).astype(np.int64) % n_track
            s[5] += np.where(2 * d > n_track, d - n_track, d)
        s[6] = np.where((s[6] < 0) & (ac > cte_limit), float(t), s[6])
        s[7] += hist[t, REC_STATUS] != 0
    return s


def check_summary(res, n_track, cte_limit):
    """Rows 0, 2, 4, 5, 6, 7 equal; rows 1 and 3 -- running sums of `steps` terms -- within steps x 2 ulp of the sum."""
    hist, summary = res["hist"], res["summary"]
    ref = summary_from_hist(hist, n_track, cte_limit)
    for r in (0, 2, 4, 5, 6, 7):
        assert np.array_equal(summary[r], ref[r]), (r, summary[r], ref[r])
    for r in (1, 3):
        assert (np.abs(summary[r] - ref[r]) <= hist.shape[0] * 2 * np.spacing(np.abs(ref[r]))).all(), r
    assert np.array_equal(res["status"], hist[:, REC_STATUS].max(0).astype(np.int32))
    assert np.array_equal(res["iters"], hist[:, REC_ITERS].sum(0).astype(np.int32))


def oracle_check_steps(cfgname, over, params, waypoints, hist, extra, cars=None):
    """On every recorded step, the oracle's telemetry handler on the recorded car and window: the same status, the steer within
    TOL_STEER / max_steering and the throttle within 1e-5.  -> (max |d steer| [rad], max |d throttle|)."""
    steps, _, B = hist.shape
    cars = range(B) if cars is None else cars
    d_steer = d_thr = 0.0
    for t in range(steps):
        px, py = window_points(waypoints, hist[t, REC_K].astype(np.int64))
        for i in cars:
            cfg = O.load_config(cfgname, **over)          # run() mutates the yaw bounds of its Config, like the reference
            st, steer, thr, _ = O.telemetry_handler(cfg, hist[t, :6, i], px[:, i], py[:, i], extra)
            assert st == int(hist[t, REC_STATUS, i]), (t, i, st, hist[t, REC_STATUS, i])
            if st == 0:
                d_steer = max(d_steer, abs(steer - hist[t, REC_CMD, i]) * params.max_steering)
                d_thr = max(d_thr, abs(thr - hist[t, REC_CMD + 1, i]))
    assert d_steer <= TOL_STEER and d_thr <= TOL_THROTTLE, (d_steer, d_thr)
    return d_steer, d_thr


# ---- the device side (tests/test_drive*_gpu.py) --------------------------------------------------------------------------------------
CHILD_TIMEOUT_S = 120
FORMS = {"device": "mpc_drive_batch_device", "fused": "mpc_drive_batch_device_fused", "host": "mpc_drive_batch_host"}
ENTRY_ARGS = {"": (), "model": ("model",), "latency": ("model", "latency"), "horizon": ("model", "horizon", "latency"),
              "plant": ("model", "horizon", "latency", "plant")}       # what each entry point takes between `weights` and `opts`
HZ_PAD = -999          # what the horizon array holds from column B on
KEYS = ("car", "summary", "hist", "status", "iters")


def to_device(a, dev, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def fast_params(pkg, golden_dir, **over):
    return pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), **dict(dict(N=10), **over))


def device_drive(pkg, params, waypoints, car, steps, dev, model=None, horizon=None, latency=None, plant=None, form="device", entry="plant", warm=0,
                 weights=None, hist=True, pad=3, opts_over=None, opts=None, mpc=None):
    """A drive entry point through the raw ABI with ld = B + pad: the symbol FORMS[form] + "_" + entry ("": the one without a suffix),
    called with exactly that symbol's arguments (ENTRY_ARGS; each array may be None: NULL; an array the symbol does not take must be
    None).  Inputs hold NaN (horizon: HZ_PAD) from column B on, outputs the sentinels everywhere before the call.  opts: the call's
    MpcDriveOpts (None: the defaults with warm_start = warm and opts_over).  -> the arrays cut to B, after checking that nothing behind
    column B was written; and the handle's mpc_drive_info.  mpc: a live handle to use (its info then counts every call made on it)."""
    import torch
    lib = pkg.library()
    B = car.shape[1]
    ld = B + pad
    tx, ty = track_of(waypoints)
    opts = opts if opts is not None else pkg.drive_opts_default(params, warm_start=warm, **(opts_over or {}))
    given = {"model": model, "horizon": horizon, "latency": latency, "plant": plant}
    assert all(v is None for k, v in given.items() if k not in ENTRY_ARGS[entry]), entry

    def wide(a, fill=np.nan):
        if a is None:
            return None
        w = np.full((a.shape[0], ld), fill); w[:, :B] = a
        return w
    h_car, h_w = wide(car), wide(weights)
    h_x = {k: wide(v) for k, v in given.items() if k != "horizon"}
    h_x["horizon"] = None
    if horizon is not None:
        h_x["horizon"] = np.full(ld, HZ_PAD, dtype=np.int32); h_x["horizon"][:B] = horizon
    h_sum = np.full((NSUM, ld), SENTINEL); h_hist = np.full((steps, REC, ld), SENTINEL) if hist else None
    h_st = np.full(ld, ISENTINEL, dtype=np.int32); h_it = np.full(ld, ISENTINEL, dtype=np.int32)
    call = getattr(lib, FORMS[form] + ("_" + entry if entry else ""))
    own = mpc is None
    if own:
        mpc = pkg.BatchedMPC(params, max(B, 1), device=0)
    try:
        if form == "host":
            p = lambda a: a.ctypes.data if a is not None else None
            ex = [p(h_x[k]) for k in ENTRY_ARGS[entry]]
            rc = call(mpc._h, B, ld, steps, p(h_car), p(tx), p(ty), len(tx), p(h_w), *ex, C.byref(opts), None, p(h_sum), p(h_hist), p(h_st), p(h_it))
            assert rc == 0, lib.mpc_last_error()
            got = {"car": h_car, "summary": h_sum, "hist": h_hist, "status": h_st, "iters": h_it}
        else:
            dd = lambda a, dt=np.float64: to_device(a, dev, dt) if a is not None else None
            d = {"car": dd(h_car), "summary": dd(h_sum), "hist": dd(h_hist), "status": dd(h_st, np.int32), "iters": dd(h_it, np.int32)}
            d_tx, d_ty, d_w = dd(tx), dd(ty), dd(h_w)
            d_x = {k: dd(v, np.int32 if k == "horizon" else np.float64) for k, v in h_x.items()}
            p = lambda t: t.data_ptr() if t is not None else None
            ex = [p(d_x[k]) for k in ENTRY_ARGS[entry]]
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


def same(a, b, keys=KEYS, cars=None):
    """bitwise, NaN == NaN included (a contained car may hold one in both)"""
    for k in keys:
        if a[k] is None or b[k] is None:      # (a call without hist: everything else is compared)
            continue
        x, y = (a[k], b[k]) if cars is None else (a[k][..., cars], b[k][..., cars])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def child_main(path):
    """Runs in the child: the batches of the case function named in the spec -- "module.function", called with (pkg, params, waypoints)
    -> [(tag, car, the per-car arrays and entry of device_drive)] -- on the device, cold and warm, results into an .npz.  Every drive is
    one call; nothing is retried."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    import torch
    pkg = G.load_package()
    spec = json.load(open(path + ".json"))
    gd = os.path.join(ROOT, "tests", "golden")
    params = fast_params(pkg, gd, **spec["params_over"])
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    module, func = spec["case"].rsplit(".", 1)
    dev = torch.device("cuda:0")
    out = {}
    for warm in (0, 1):
        for tag, car, kw in getattr(importlib.import_module(module), func)(pkg, params, wp):
            r = device_drive(pkg, params, wp, car, 4, dev, warm=warm, form="fused" if spec["fused"] else "device", **kw)
            for k in KEYS:
                out["%d/%s/%s" % (warm, tag, k)] = r[k]
            out["%d/%s/info" % (warm, tag)] = np.array([r["info"]["fused_launches"], r["info"]["stepwise_loops"]])
    np.savez(path, **out)


def run_in_child(case, fused, wave_max_batch=None, timeout=CHILD_TIMEOUT_S):
    """The case function `case` ("module.function", see child_main) in a fresh child process -> {(warm, tag): the arrays of
    device_drive}; a child that does not end within `timeout` seconds fails the caller (subprocess.TimeoutExpired) after it has been
    killed; the parent checks the exit status"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "case.npz")
        over = {} if wave_max_batch is None else {"wave_max_batch": int(wave_max_batch)}
        json.dump({"case": case, "params_over": over, "fused": bool(fused)}, open(path + ".json", "w"))
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
