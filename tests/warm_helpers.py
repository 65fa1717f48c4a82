"""Helpers of the warm-start tests (test infrastructure): the TEST-ONLY CPU build of the warm start (mpc_twin_solve of
tests/host_twin) and the closed loops both test files run."""
import ctypes as C
import os
import subprocess

import numpy as np

from helpers import ROOT, load_twin, vp

load_warm_twin = load_twin


def twin_warm_solve(twin, params, batch, opts, warm=None, warm_status=None, want_warm=True, inplace=False):
    """Solver::solve_warm of the device header, CPU build, with the arguments of mpc_solve_batch_host_warm.  inplace: warm_out is
    the `warm` array itself and warm_status the returned status array."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    st, cf, yl, yh = f(batch["state"]), f(batch["coeffs"]), f(batch["yaw_lo"]), f(batch["yaw_hi"])
    B = st.shape[1]
    rows = (params.N - 1) * 22
    out = np.zeros((9, B)); status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    if warm is not None:
        warm = warm if inplace else f(warm).copy()
        assert warm.shape == (rows, B) and warm.flags.c_contiguous and warm.dtype == np.float64
    wout = warm if inplace else (np.zeros((rows, B)) if want_warm else None)
    if inplace and warm_status is not None:
        status = warm_status
    elif warm_status is not None:
        warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
    rc = twin.mpc_twin_solve(C.byref(params), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), None, None, vp(warm),
                             vp(warm_status), vp(wout), C.c_int64(B), C.byref(opts), C.c_int(0), vp(out), None, vp(status), vp(iters))
    assert rc == 0
    return {"out": out, "status": status, "iters": iters, "warm": wout}


def twin_closed_loop(twin, params, sc, steps, opts, warm_start):
    """`steps` closed-loop solves per car (src/test.cpp:79-111), step 1 cold, the others warm-started from the step before (or cold
    too) -> hist [steps, 9, B], status and iterations of every solve [steps, B]."""
    B = sc["state"].shape[1]
    hist = np.zeros((steps, 9, B)); sst = np.zeros((steps, B), dtype=np.int32); sit = np.zeros((steps, B), dtype=np.int32)
    st = np.array(sc["state"], dtype=np.float64, copy=True)
    warm, wstat = None, None
    for k in range(steps):
        r = twin_warm_solve(twin, params, dict(state=st, coeffs=sc["coeffs"], yaw_lo=sc["yaw_lo"], yaw_hi=sc["yaw_hi"]), opts,
                            warm=warm if warm_start else None, warm_status=wstat if warm_start else None)
        hist[k] = r["out"]; sst[k] = r["status"]; sit[k] = r["iters"]
        st = r["out"][:6].copy(); warm, wstat = r["warm"], r["status"]
    return hist, sst, sit


def golden_batches(pkg, golden_dir):
    """The instances of tests/golden/scipy_cross_solve.json, one batch per configuration: (config name, params, batch)."""
    from helpers import load_golden
    gold = load_golden("scipy_cross_solve.json")
    for cfgname in ("config-stable.json", "config-fast.json"):
        cases = [c for c in gold["cases"] if c["config"] == cfgname]
        params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
        b = {"state": np.array([c["state"] for c in cases]).T.copy(), "coeffs": np.array([c["coef"] for c in cases]).T.copy(),
             "yaw_lo": np.array([c["yaw_lo"] for c in cases]), "yaw_hi": np.array([c["yaw_hi"] for c in cases])}
        yield cfgname, params, b


def garbage_warm(params, good):
    """Two spoilt copies of a warm buffer: all NaN, and every bounded quantity (psi, v, delta, a) far outside its bounds."""
    nan = np.full_like(good, np.nan)
    far = good.copy()
    for k in range(params.N - 1):
        for f in (2, 3, 6, 7):
            far[k * 22 + f] = 1e3
    return nan, far


def build_drop_in_warm(pkg, out_dir=None):
    """Compile tests/cpp/drop_in_warm_test.cpp against include/mpc_drop_in.hpp and the product library -> path of the binary."""
    import tempfile
    pkg.library()
    out = os.path.join(out_dir or tempfile.mkdtemp(prefix="dropin_warm"), "drop_in_warm_test")
    libdir = os.path.dirname(pkg.library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "drop_in_warm_test.cpp"), "-L", libdir, "-lmpc_amd", "-Wl,-rpath," + libdir])
    return out
