"""Helpers of the tests of the track drive under noise (test infrastructure): the TEST-ONLY CPU build of the mpc_drive_*_noise calls
(tests/drive_twin/noise_drive_twin.cpp, a library of its own compiled from here), an independent numpy statement of the random stream
(integer Philox4x32-10, np.log, np.sqrt, np.cos / np.sin) with the bound a draw is held to, the stated (seed, step) pairs and noise
columns, and the calls both test files make -- the twin's, the raw-ABI device call, and the child process for columns no caller
should send."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

from helpers import ROOT, vp

NNOISE = 7
SEED, POS, PSI, SPEED, STEER, DRIFT, DROP = range(NNOISE)
Z_X, Z_Y, Z_PSI, Z_SPEED, Z_STEER, Z_DRIFT, U_DROP = range(7)
SENTINEL, ISENTINEL = -7777.25, -12345
SUCCESS, MAXITER, LINESEARCH, INFEASIBLE, ACCEPTABLE = 0, 1, 2, 3, 6      # MPC_STATUS_*
CSRC = os.path.join(ROOT, "carnd-mpc-project_amd", "csrc")
INC = os.path.join(ROOT, "include")
TWIN_DIR = os.path.join(ROOT, "tests", "drive_twin")
TWIN_SRC = os.path.join(TWIN_DIR, "noise_drive_twin.cpp")
TWIN_FLAGS = ["-x", "c++", "-no-hip-rt", "-O2", "-mfma", "-ffp-contract=on"]      # (budget_helpers.load_budget_drive_twin's compile line)
TWIN_DEPS = [TWIN_SRC] + [os.path.join(CSRC, h) for h in ("mpc_core.h", "mpc_run_core.h", "mpc_drive_core.h")] + [
    os.path.join(INC, h) for h in ("mpc_amd.h", "mpc_amd_budget.h", "mpc_amd_drive.h", "mpc_amd_noise.h")]

# The bound of one normal, |z - z_ref| <= rad * DRAW_REL with rad = sqrt(-2 ln u_a) as the reference has it.  z = rad * t, t the cosine
# or sine of theta = fl(6.283185307179586 * u_b) -- one rounded product, the same double on both sides.  Against the exact value
#   the library's side: t off by at most D_SINCOS absolute (tests/test_math_conformance.py: f64 sincos abs 4e-16, |x| < 1e9; theta < 6.3),
#     ln u_a off by at most D_LOG relative (f64 flog rel 2.3e-16), hence rad by D_LOG / 2 relative, plus half an ulp for the correctly
#     rounded square root and half an ulp for the product rad * t;
#   numpy's side: one ulp (2^-52 relative; of t at most 2^-52 absolute) for np.log, np.cos and np.sin each, hence rad off by 2^-53
#     relative, t by 2^-52 absolute, plus the same two half ulps;
# and |t| <= 1, so everything is at most rad times
#   D_SINCOS + D_LOG / 2 + (1 + 1) 2^-53 [library: sqrt, product] + (1 + 2 + 1 + 1) 2^-53 [numpy: log / 2, cos or sin, sqrt, product]
# plus products of two such terms (< 1e-30), for which one more 2^-53 stands: D_SINCOS + D_LOG / 2 + 8 * 2^-53.
D_SINCOS, D_LOG = 4e-16, 2.3e-16      # the bounds tests/test_math_conformance.py holds f64 fsincos and flog to
DRAW_REL = D_SINCOS + D_LOG / 2 + 8 * 2.0 ** -53

_twin = None


def load_noise_drive_twin():
    """tests/drive_twin/noise_drive_twin.cpp -> libnoise_drive_twin.so, by budget_helpers.load_budget_drive_twin's compile line: with
    noise = NULL and seen = NULL its bits are compared with that library's."""
    global _twin
    if _twin is None:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's own comes first, as in drive_helpers.load_drive_twin)
        except ImportError:
            pass
        out = os.path.join(TWIN_DIR, "libnoise_drive_twin.so")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in TWIN_DEPS):
            tmp = out + ".%d.tmp" % os.getpid()
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc] + TWIN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", INC, "-I", CSRC, "-o", tmp, TWIN_SRC])
            os.replace(tmp, out)
        _twin = C.CDLL(out)
        _twin.mpc_noise_drive_twin_draw.argtypes = [C.c_double, C.c_int32, C.c_void_p]
    return _twin


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64) if a is not None else None


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32) if a is not None else None


# ---- the random stream, independently ----------------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def np_philox4x32(ctr, key):
    """Philox4x32-10 on arrays: ctr [4, n], key [2, n] of integers below 2^32 -> [4, n] uint64 holding 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c)


def np_draw(seed, step):
    """The seven values of every (seed, step) pair, seed / step [n] integers -> (draw [7, n], rad [7, n]: the radius each normal was
    scaled with, 0 in the u_drop row)"""
    seed = np.asarray(seed, dtype=np.uint64)
    step = np.asarray(step, dtype=np.uint64)
    key = [seed & MASK, seed >> np.uint64(32)]
    zero = np.zeros_like(step)
    uni = lambda r: (r.astype(np.float64) + 0.5) * 2.0 ** -32

    def pair(ra, rb):
        rad = np.sqrt(-2.0 * np.log(uni(ra)))
        th = 6.283185307179586 * uni(rb)
        return rad * np.cos(th), rad * np.sin(th), rad
    b0, b1 = np_philox4x32([step, zero, zero, zero], key), np_philox4x32([step, zero + np.uint64(1), zero, zero], key)
    zx, zy, r0 = pair(b0[0], b0[1])
    zp, zs, r1 = pair(b0[2], b0[3])
    zt, zd, r2 = pair(b1[0], b1[1])
    return np.stack([zx, zy, zp, zs, zt, zd, uni(b1[2])]), np.stack([r0, r0, r1, r1, r2, r2, np.zeros_like(r0)])


def stated_pairs():
    """seeds 1000 .. 1255 x steps 0 .. 255 (seed-major: pair s * 256 + t), then seeds 0, 2^32 - 1, 2^32, 2^53 - 1 at steps 0 and
    2^31 - 1 -> seed [65544] float64, step [65544] int32; the first 65536 are the grid"""
    s, t = np.meshgrid(np.arange(1000, 1256), np.arange(256), indexing="ij")
    es, et = np.meshgrid([0, 2 ** 32 - 1, 2 ** 32, 2 ** 53 - 1], [0, 2 ** 31 - 1], indexing="ij")
    return (np.concatenate([s.ravel(), es.ravel()]).astype(np.float64), np.concatenate([t.ravel(), et.ravel()]).astype(np.int32))


def lib_draws(lib, seed, step, fn="mpc_drive_noise_draw"):
    """mpc_drive_noise_draw (or the twin's) on every pair -> [7, n]"""
    out = np.empty((len(seed), 7))
    f = getattr(lib, fn)
    row = np.empty(7)
    for j in range(len(seed)):
        rc = f(C.c_double(seed[j]), C.c_int32(int(step[j])), row.ctypes.data)
        assert rc == 0, (rc, seed[j], step[j])
        out[j] = row
    return np.ascontiguousarray(out.T)


# ---- the columns -------------------------------------------------------------------------------------------------------------------
MODERATE = {POS: 0.3, PSI: 0.02, SPEED: 1.0, STEER: 0.01, DRIFT: 0.3, DROP: 0.1}      # all seven rows non-zero with the seeds


def noise_columns(B, rows=MODERATE, seed0=5000):
    """[7, B]: seeds seed0 + 7 i (car i), every other row the value of `rows` (a row left out: 0)"""
    a = np.zeros((NNOISE, B))
    a[SEED] = seed0 + 7 * np.arange(B)
    for r, v in rows.items():
        a[r] = v
    return a


GROUPS = ({POS: 0.5}, {PSI: 0.03, SPEED: 2.0}, {STEER: 0.02, DRIFT: 0.5, DROP: 0.3}, MODERATE)      # the four interleaved groups of the mixed batch


def mixed_columns(B):
    """car i has the sigma rows of GROUPS[i % 4] and its own seed"""
    a = noise_columns(B, {})
    for g, rows in enumerate(GROUPS):
        for r, v in rows.items():
            a[r, g::4] = v
    return a


UNUSABLE = ([(r, np.nan) for r in range(NNOISE)] + [(r, np.inf) for r in range(NNOISE)] + [(r, -1.0) for r in range(POS, DRIFT + 1)] +
            [(DROP, 1.5), (DROP, -0.1), (SEED, 0.5), (SEED, -1.0), (SEED, 2.0 ** 53)])      # (row, value): one per car among clean cars


def unusable_batch(clean):
    """clean [7, B] -> (dirty, bad): the defects of UNUSABLE in every second column from 1 on (B >= 2 * len(UNUSABLE) + 1)"""
    dirty = clean.copy()
    bad = 1 + 2 * np.arange(len(UNUSABLE))
    assert bad[-1] < clean.shape[1]
    for c, (r, v) in zip(bad, UNUSABLE):
        dirty[r, c] = v
    return dirty, bad


def check_unusable(got, ref, zero, bad, handler_status=None):
    """The rule of a column that cannot be used: the bad cars are driven as with the zero column (`zero`: the call with those cars'
    columns zero) except that every step the handler ended SUCCESS or ACCEPTABLE is INFEASIBLE in hist row 10, summary row 7 and the
    folded status; iterations untouched; no not-a-number; every other car is bitwise what it is without the defect (`ref`)."""
    B = got["status"].shape[0]
    good = np.setdiff1d(np.arange(B), bad)
    for k in ("car", "summary", "hist", "seen", "status", "iters"):
        if got.get(k) is None:
            continue
        assert np.isfinite(got[k]).all(), k
        assert got[k][..., good].tobytes() == ref[k][..., good].tobytes(), ("neighbours", k)
    h, z = got["hist"][..., bad], zero["hist"][..., bad]
    st = z[:, 10]
    want = np.where((st == SUCCESS) | (st == ACCEPTABLE), float(INFEASIBLE), st)
    assert np.array_equal(h[:, 10], want)
    assert np.array_equal(np.delete(h, 10, axis=1), np.delete(z, 10, axis=1))      # the drive itself: the zero column's, bit for bit
    assert np.array_equal(got["car"][:, bad], zero["car"][:, bad]) and np.array_equal(got["iters"][bad], zero["iters"][bad])
    if got.get("seen") is not None:
        assert np.array_equal(got["seen"][..., bad], zero["seen"][..., bad])
    assert np.array_equal(got["summary"][:7, bad], zero["summary"][:7, bad])
    assert np.array_equal(got["summary"][7, bad], (want != SUCCESS).sum(0).astype(np.float64))
    assert np.array_equal(got["status"][bad], want.max(0).astype(np.int32))      # (the fold is the worst code: the largest)
    if handler_status is not None:
        assert np.array_equal(handler_status[:, bad].astype(np.float64), st)      # the handler's own status is untouched


# ---- the twin ----------------------------------------------------------------------------------------------------------------------
def twin_noise_drive(twin, params, waypoints, car, steps, opts, warm_opts, noise=None, seen=True, budget=None, model=None, horizon=None, latency=None,
                     plant=None, weights=None, pad=0):
    """mpc_noise_drive_twin with the arguments of mpc_drive_batch_host_noise and ld = B + pad, each per-car array or None (NULL) ->
    car, summary, hist [steps, 13, B], seen [steps, 4, B] or None, status, iters, and handler_status [steps, B]."""
    from drive_helpers import NSUM, REC, track_of
    tx, ty = track_of(waypoints)
    B = np.asarray(car).shape[1]
    ld = B + pad

    def wide(a, fill=np.nan, dtype=np.float64):
        if a is None:
            return None
        a = np.atleast_2d(np.asarray(a, dtype=dtype))
        w = np.full((a.shape[0], ld), fill, dtype=dtype); w[:, :B] = a
        return w
    h_car, h_m, h_l, h_p, h_n, h_w = (wide(a) for a in (car, model, latency, plant, noise, weights))
    h_hz, h_bg = (wide(a, -999, np.int32) for a in (horizon, budget))
    summary = np.full((NSUM, ld), SENTINEL); hist = np.full((steps, REC, ld), SENTINEL)
    sn = np.full((steps, 4, ld), SENTINEL) if seen else None
    status = np.full(ld, ISENTINEL, dtype=np.int32); iters = np.full(ld, ISENTINEL, dtype=np.int32)
    hs = np.full((steps, ld), ISENTINEL, dtype=np.int32)
    rc = twin.mpc_noise_drive_twin(C.byref(params), C.c_int64(B), C.c_int64(ld), C.c_int(steps), vp(h_car), vp(tx), vp(ty), C.c_int(len(tx)), vp(h_w), vp(h_m),
                                   vp(h_hz), vp(h_bg), vp(h_l), vp(h_p), vp(h_n), C.byref(opts), C.byref(warm_opts), vp(summary), vp(hist), vp(sn),
                                   vp(status), vp(iters), vp(hs))
    assert rc == 0, rc
    for a in (summary, hist, sn):
        assert a is None or (a[..., B:] == SENTINEL).all()
    return {"car": h_car[:, :B].copy(), "summary": summary[:, :B].copy(), "hist": hist[..., :B].copy(), "seen": sn[..., :B].copy() if seen else None,
            "status": status[:B].copy(), "iters": iters[:B].copy(), "handler_status": hs[:, :B].copy()}


def twin_noise_handler(twin, params, waypoints, told, k, opts, warm_opts, budget=None, comp=None, model=None, horizon=None, weights=None, warm=None,
                       warm_status=None, want_warm=False):
    """mpc_noise_drive_twin_handler: one handler call of the CPU build on what it is told [6, B] with the windows that start at k ->
    cmd, status, iters, cte_epsi, warm (the rows of params.N)."""
    from drive_helpers import track_of
    tx, ty = track_of(waypoints)
    told = _f(told)
    B = told.shape[1]
    rows = (params.N - 1) * 22
    cmd = np.zeros((2, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32); ce = np.zeros((2, B))
    wout = np.zeros((rows, B)) if (want_warm or warm is not None) else None
    rc = twin.mpc_noise_drive_twin_handler(C.byref(params), C.c_int64(B), C.c_int64(B), vp(told), vp(_f(comp)), vp(_i(k)), vp(tx), vp(ty), C.c_int(len(tx)),
                                           vp(_f(weights)), vp(_f(model)), vp(_i(horizon)), vp(_i(budget)), C.byref(opts), vp(_f(warm)), vp(_i(warm_status)),
                                           vp(wout), C.c_int64(B), C.byref(warm_opts), vp(cmd), vp(status), vp(iters), vp(ce))
    assert rc == 0, rc
    return {"cmd": cmd, "status": status, "iters": iters, "cte_epsi": ce, "warm": wout}


KEYS = ("car", "summary", "hist", "seen", "status", "iters")


def same(a, b, keys=KEYS, cars=None, what=""):
    """bitwise, NaN == NaN included; a key either side does not have is skipped"""
    for k in keys:
        if a.get(k) is None or b.get(k) is None:
            continue
        x, y = (a[k], b[k]) if cars is None else (a[k][..., cars], b[k][..., cars])
        assert x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, k)


# ---- the device side (tests/test_drive_noise_gpu.py) --------------------------------------------------------------------------------
NOISE_FORMS = {"device": "mpc_drive_batch_device_noise", "fused": "mpc_drive_batch_device_fused_noise", "host": "mpc_drive_batch_host_noise"}
BUDGET_FORMS = {"device": "mpc_drive_batch_device_budget", "fused": "mpc_drive_batch_device_fused_budget", "host": "mpc_drive_batch_host_budget"}


def device_noise_drive(pkg, params, waypoints, car, steps, dev, noise=None, seen=True, budget=None, model=None, horizon=None, latency=None, plant=None,
                       form="device", entry="noise", warm=0, weights=None, hist=True, pad=3, mpc=None, expect=0):
    """A _noise drive entry point through the raw ABI with ld = B + pad (pad < 0: a call to be refused; the arrays are B wide; entry
    "budget": the form it extends; noise must be None and seen False): inputs hold NaN (the int arrays -999) from column B on, outputs the sentinels everywhere before the call -> the
    arrays cut to B, after checking that nothing behind column B was written; and the handle's mpc_drive_info.  expect != 0: the call
    must be refused with that code and write nothing -> the refusal's text."""
    import torch
    import drive_helpers as D
    lib = pkg.library()
    B = car.shape[1]
    ld, width = B + pad, B + max(pad, 0)
    tx, ty = D.track_of(waypoints)
    opts = pkg.drive_opts_default(params, warm_start=warm)
    assert entry == "noise" or (noise is None and not seen)
    assert pad >= 0 or expect

    def wide(a, fill=np.nan, dtype=np.float64):
        if a is None:
            return None
        a = np.atleast_2d(np.asarray(a, dtype=dtype))
        w = np.full((a.shape[0], width), fill, dtype=dtype); w[:, :B] = a
        return w
    h_in = [wide(car), tx, ty, wide(weights), wide(model), wide(horizon, D.HZ_PAD, np.int32), wide(budget, D.HZ_PAD, np.int32), wide(latency), wide(plant),
            wide(noise)]
    h_out = {"summary": np.full((D.NSUM, width), SENTINEL), "hist": np.full((steps, D.REC, width), SENTINEL) if hist else None,
             "seen": np.full((steps, 4, width), SENTINEL) if seen else None, "status": np.full(width, ISENTINEL, dtype=np.int32),
             "iters": np.full(width, ISENTINEL, dtype=np.int32)}
    call = getattr(lib, (NOISE_FORMS if entry == "noise" else BUDGET_FORMS)[form])
    own = mpc is None
    if own:
        mpc = pkg.BatchedMPC(params, max(B, 1), device=0)
    try:
        if form == "host":
            p = lambda a: a.ctypes.data if a is not None else None
            x, y, tail = h_in, h_out, ()
        else:
            x = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None for a in h_in]
            y = {k: (torch.from_numpy(v).to(dev) if v is not None else None) for k, v in h_out.items()}
            p = lambda t: t.data_ptr() if t is not None else None
            tail = (C.c_void_p(torch.cuda.current_stream(dev).cuda_stream),)
        nz, sn = ((p(x[9]),), (p(y["seen"]),)) if entry == "noise" else ((), ())
        rc = call(mpc._h, B, ld, steps, p(x[0]), p(x[1]), p(x[2]), len(tx), *[p(t) for t in x[3:9]], *nz, C.byref(opts), None, p(y["summary"]), p(y["hist"]),
                  *sn, p(y["status"]), p(y["iters"]), *tail)
        assert rc == expect, (rc, lib.mpc_last_error())
        if form != "host":
            torch.cuda.synchronize()
            y = {k: (v.cpu().numpy() if v is not None else None) for k, v in y.items()}
            x[0] = x[0].cpu().numpy()
        info = mpc.drive_info()
    finally:
        if own:
            mpc.close()
    got = dict(y, car=x[0])
    if expect:
        assert all(v is None or (v == (ISENTINEL if v.dtype == np.int32 else SENTINEL)).all() for v in y.values()), "a refused call wrote"
        assert got["car"][:, :B].tobytes() == np.ascontiguousarray(car, dtype=np.float64).tobytes(), "a refused call moved the cars"
        return lib.mpc_last_error().decode()
    assert np.isnan(got["car"][:, B:]).all()
    for k, v in y.items():
        assert v is None or (v[..., B:] == (ISENTINEL if v.dtype == np.int32 else SENTINEL)).all(), k
    out = {k: (v[..., :B].copy() if v is not None else None) for k, v in got.items()}
    assert (out["summary"] != SENTINEL).all() and (out["status"] != ISENTINEL).all() and (out["iters"] != ISENTINEL).all()
    assert out["seen"] is None or (out["seen"] != SENTINEL).all()
    out["info"] = info
    return out


def device_draws(pkg, mpc, dev, seed, step):
    """mpc_debug_drive_noise_device on the pairs -> [7, n]"""
    import torch
    n = len(seed)
    d_s, d_t = torch.from_numpy(_f(seed)).to(dev), torch.from_numpy(_i(step)).to(dev)
    d_o = torch.full((7, n), SENTINEL, dtype=torch.float64, device=dev)
    rc = pkg.library().mpc_debug_drive_noise_device(mpc._h, n, d_s.data_ptr(), d_t.data_ptr(), d_o.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, pkg.library().mpc_last_error()
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


# ---- columns no caller should send, in a child process under its own time limit (drive_helpers.run_in_child's arrangement) -----------
CHILD_TIMEOUT_S = 120
CHILD_CARS, CHILD_STEPS = 65, 4


def child_cases(pkg, params, waypoints):
    """-> (car, clean, dirty, bad, zeroed): the stated cars, the moderate columns, those with the defects of UNUSABLE, and the clean
    ones with the bad cars' columns zero"""
    car = pkg.scenarios.track_starts(CHILD_CARS, params, waypoints, seed=6)
    clean = noise_columns(CHILD_CARS)
    dirty, bad = unusable_batch(clean)
    zeroed = clean.copy(); zeroed[:, bad] = 0.0
    return car, clean, dirty, bad, zeroed


def child_main(path):
    """Runs in the child: the three batches of child_cases on the device, cold and warm, results into an .npz.  Every drive is one
    call; nothing is retried."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    import torch
    from drive_helpers import fast_params
    pkg = G.load_package()
    spec = json.load(open(path + ".json"))
    gd = os.path.join(ROOT, "tests", "golden")
    params = fast_params(pkg, gd, **spec["params_over"])
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    dev = torch.device("cuda:0")
    car, clean, dirty, bad, zeroed = child_cases(pkg, params, wp)
    out = {}
    for warm in (0, 1):
        for tag, nz in (("ref", clean), ("got", dirty), ("zero", zeroed)):
            r = device_noise_drive(pkg, params, wp, car, CHILD_STEPS, dev, noise=nz, warm=warm, form="fused" if spec["fused"] else "device")
            for k in KEYS:
                out["%d/%s/%s" % (warm, tag, k)] = r[k]
            out["%d/%s/info" % (warm, tag)] = np.array([r["info"]["fused_launches"], r["info"]["stepwise_loops"]])
    np.savez(path, **out)


def run_in_child(fused, wave_max_batch=None, timeout=CHILD_TIMEOUT_S):
    """child_main in a fresh child process -> {(warm, tag): the arrays of device_noise_drive}; a child that does not end within
    `timeout` seconds fails the caller (subprocess.TimeoutExpired) after it has been killed; the parent checks the exit status"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "case.npz")
        over = {} if wave_max_batch is None else {"wave_max_batch": int(wave_max_batch)}
        json.dump({"params_over": over, "fused": bool(fused)}, open(path + ".json", "w"))
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
