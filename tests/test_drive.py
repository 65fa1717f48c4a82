"""Track driving (include/mpc_amd_drive.h), checked without a GPU: the CPU build of the stepwise definition (tests/drive_twin:
mpc_drive_core.h around the handler's own functions) against numpy's window rule (run_warm_helpers.pick_window), against the plant as
a composition of the oracle's Vehicle::move, against the oracle's telemetry handler on every recorded step, and its summary rows
against the records; and what the ABI says without a device: the defaults, the declarations, the refusals that need no handle."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import drive_helpers as D
import oracle_lib as O
from run_warm_helpers import pick_window

WINDOW_SEED = 5      # chosen so that none of the 4 096 random points sits on a tie (asserted in test_window)


@pytest.fixture(scope="module")
def twin():
    return D.load_drive_twin()


def test_window(twin, waypoints):
    """4 096 random points within 30 m of the lake track, and every waypoint itself, against pick_window.  A point may be left out
    only where numpy's two smallest distances differ by less than 1e-9 relative or |dot| < 1e-9; none of the random points is."""
    wp = np.asarray(waypoints, dtype=np.float64)
    n = len(wp)
    g = np.random.default_rng(WINDOW_SEED)
    at = g.integers(0, n, 4096)
    r, phi = 30.0 * np.sqrt(g.uniform(0, 1, 4096)), g.uniform(0, 2 * np.pi, 4096)
    x = np.concatenate([wp[at, 0] + r * np.cos(phi), wp[:, 0]]); y = np.concatenate([wp[at, 1] + r * np.sin(phi), wp[:, 1]])
    k = D.twin_window(twin, wp, x, y)
    assert ((k >= 0) & (k < n)).all()
    px, py = pick_window(wp, x, y)
    qx, qy = D.window_points(wp, k)
    same = (px == qx).all(0) & (py == qy).all(0)
    d2 = np.sort(((np.stack([x, y], 1)[:, None, :] - wp[None, :, :]) ** 2).sum(2), axis=1)
    j = np.argmin(((np.stack([x, y], 1)[:, None, :] - wp[None, :, :]) ** 2).sum(2), axis=1)
    dot = ((np.stack([x, y], 1) - wp[j]) * (wp[(j + 1) % n] - wp[j])).sum(1)
    may_skip = (d2[:, 1] - d2[:, 0] < 1e-9 * d2[:, 1]) | (np.abs(dot) < 1e-9)
    assert not may_skip[:4096].any(), "choose another WINDOW_SEED: %d random points sit on a tie" % may_skip[:4096].sum()
    assert same[:4096].all()                                    # cap: 0 left out
    assert (same | may_skip).all()
    # a waypoint itself: j is that waypoint, the dot product is 0, not > 0: the window starts one before it
    assert np.array_equal(k[4096:], (np.arange(n) - 1) % n)
    # a position that is not finite: j = 0, and the dot product is no number either, so k = n - 1; the call returns
    bad = D.twin_window(twin, wp, np.array([np.nan, np.inf, 0.0]), np.array([0.0, 0.0, -np.inf]))
    assert np.array_equal(bad, [n - 1] * 3)


@pytest.mark.parametrize("sub_old,sub_new", [(10, 2), (0, 10), (3, 0)])
def test_plant(pkg, twin, golden_dir, sub_old, sub_new):
    """256 cars against the composition of O.vehicle_move.  The bound, per row: 4 x substeps x 1 ulp of max(1, |value|).  One substep of
    Vehicle::move (Vehicle.cpp:145-168) performs, for the row with the most operations (x or y): dist = v * dt, cos / sin(psi),
    dist * cos, x + that -- four operations, each rounded once, each rounding at most 1 ulp of a value no larger than the row's own
    (dist <= 0.4 m against |x| of tens of metres).  The two builds differ in exactly such roundings (the device header fuses the
    multiply-adds and has its own sin / cos), so after s substeps a row is at most 4 s ulp of max(1, |value|) apart; psi and the
    speed have fewer operations of their own and take the same bound."""
    B, h = 256, 0.01
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    cfg = O.load_config("config-fast.json")
    g = np.random.default_rng(11)
    car = np.stack([g.uniform(-200, 200, B), g.uniform(-200, 200, B), g.uniform(-np.pi, np.pi, B), g.uniform(10, 80, B), g.uniform(-0.4, 0.4, B),
                    g.uniform(-1, 1, B)])
    cmd = np.stack([g.uniform(-1, 1, B), g.uniform(-1, 1, B)])
    cmd[0, 3] = np.nan; cmd[1, 4] = np.inf; cmd[:, 5] = np.nan      # a reply that is not finite keeps the old command
    got = D.twin_plant(twin, params, car, cmd, sub_old, sub_new, h)
    ref = D.oracle_plant(cfg, car, cmd, params.max_steering, sub_old, sub_new, h)
    bound = 4 * (sub_old + sub_new) * np.spacing(np.maximum(1.0, np.abs(ref)))
    err = np.abs(got - ref)
    print("plant (%d, %d): max error / bound per row %s" % (sub_old, sub_new, (err / bound).max(1)))
    assert (err <= bound).all()
    keep = [3, 4, 5]
    assert np.array_equal(got[4:, keep], car[4:, keep])              # the old command is still in force
    ok = np.setdiff1d(np.arange(B), keep)
    assert np.array_equal(got[4, ok], cmd[0, ok] * params.max_steering) and np.array_equal(got[5, ok], cmd[1, ok])


@pytest.fixture(scope="module")
def loops(pkg, twin, golden_dir, waypoints):
    """16 cars x 8 steps, N = 10, config-fast and config-stable, cold and warm: computed once, shared, never changed."""
    out = {}
    for cfgname in ("config-fast.json", "config-stable.json"):
        params = pkg.params_from_json(os.path.join(golden_dir, cfgname), N=10)
        car = pkg.scenarios.track_starts(16, params, waypoints, seed=3)
        for warm in (0, 1):
            opts = pkg.drive_opts_default(params, warm_start=warm)
            out[cfgname, warm] = (params, opts, D.twin_drive(twin, params, waypoints, car, 8, opts, pkg.warm_opts_default()))
    return out


@pytest.mark.parametrize("cfgname", ["config-fast.json", "config-stable.json"])
@pytest.mark.parametrize("warm", [0, 1])
def test_loop_against_the_oracle(loops, waypoints, cfgname, warm):
    params, opts, res = loops[cfgname, warm]
    d_steer, d_thr = D.oracle_check_steps(cfgname, {"N": 10}, params, waypoints, res["hist"], opts.extra_latency)
    print("%s warm %d: max |d steer| %.3g rad, |d throttle| %.3g; statuses %s; iterations per solve %.2f" % (
        cfgname, warm, d_steer, d_thr, np.bincount(res["hist"][:, D.REC_STATUS].astype(np.int64).ravel()), res["hist"][:, D.REC_ITERS].mean()))
    # the records are the loop: the car of step t + 1 is the plant on the car and the reply of step t
    hist = res["hist"]
    assert np.isfinite(hist).all() and (hist[:, D.REC_K] == np.round(hist[:, D.REC_K])).all()
    assert (hist[1:, 4] == hist[:-1, D.REC_CMD] * params.max_steering).all() and (hist[1:, 5] == hist[:-1, D.REC_CMD + 1]).all()


@pytest.mark.parametrize("cfgname", ["config-fast.json", "config-stable.json"])
@pytest.mark.parametrize("warm", [0, 1])
def test_summary(loops, waypoints, cfgname, warm):
    params, opts, res = loops[cfgname, warm]
    D.check_summary(res, len(waypoints), opts.cte_limit)
    assert (res["summary"][5] >= 0).all() and (res["summary"][5] <= 8).all()      # the cars go forward, a few waypoints in 8 messages


def test_warm_loop_takes_fewer_iterations(loops):
    cold, warm = loops["config-fast.json", 0][2], loops["config-fast.json", 1][2]
    assert np.array_equal(cold["hist"][0], warm["hist"][0])                         # step 1 is cold either way
    assert warm["iters"].sum() < cold["iters"].sum()


def test_defaults_and_refusals_without_a_device(pkg, golden_dir):
    lib = pkg.library()
    from carnd_mpc_project_amd import _abi
    for name in _abi.DRIVE_EXPORTS:
        assert hasattr(lib, name), name
    inc = os.path.join(_abi.ROOT, "include")
    assert '#include "mpc_amd_drive.h"' in open(os.path.join(inc, "mpc_amd.h")).read()
    header = open(os.path.join(inc, "mpc_amd_drive.h")).read()
    assert set(re.findall(r"^int\s+(mpc_[a-z0-9_]+)\s*\(", header, re.M)) == set(_abi.DRIVE_EXPORTS)
    assert lib.mpc_abi_version() == 5
    for cfgname in ("config-fast.json", "config-stable.json"):
        params = pkg.params_from_json(os.path.join(golden_dir, cfgname))
        o = pkg.drive_opts_default(params)
        assert (o.size, o.npts, o.h, o.warm_start, o.extra_latency, o.cte_limit) == (C.sizeof(_abi.MpcDriveOpts), 6, 0.01, 0, 0.0, 3.0)
        assert o.sub_old == int(round(params.latency_ms / 10.0)) and o.sub_new == (2 if params.latency_ms else 10)
    p0 = params.copy(); p0.latency_ms = 0
    o = pkg.drive_opts_default(p0)
    assert (o.sub_old, o.sub_new) == (0, 10)
    assert lib.mpc_drive_opts_default(None, C.byref(o)) == -1 and lib.mpc_drive_opts_default(C.byref(params), None) == -1
    # no handle: refused before anything is touched
    a = (C.c_int64 * 2)()
    assert lib.mpc_drive_info(None, a) == -1
    assert lib.mpc_drive_batch_device(None, 1, 1, 1, None, None, None, 70, None, C.byref(o), None, None, None, None, None, None) == -1
    assert b"NULL handle" in lib.mpc_last_error()
    assert lib.mpc_drive_batch_host(None, 1, 1, 1, None, None, None, 70, None, C.byref(o), None, None, None, None, None) == -1
    # the struct and the constants as the header spells them
    names = ["MPC_DRIVE_MAX_TRACK", "MPC_DRIVE_NSUM", "MPC_DRIVE_REC", "(int)sizeof(MpcDriveOpts)", "MPC_DRIVE_SUM_FAILED", "MPC_DRIVE_REC_K"]
    src = '#include <stdio.h>\n#include "mpc_amd.h"\nint main(){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%d"] * len(names)), ", ".join(names))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", inc, "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [_abi.DRIVE_MAX_TRACK, _abi.DRIVE_NSUM, _abi.DRIVE_REC, C.sizeof(_abi.MpcDriveOpts), _abi.DRIVE_SUM_FAILED, _abi.DRIVE_REC_K]


def test_track_starts(pkg, golden_dir, waypoints):
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    car = pkg.scenarios.track_starts(512, params, waypoints, seed=1)
    assert car.shape == (6, 512) and car.dtype == np.float64 and np.isfinite(car).all()
    assert (car[3] >= 20.0).all() and (car[3] <= 60.0).all() and (car[4] == 0).all()
    wp = np.asarray(waypoints)
    d = np.sqrt(((car[:2].T[:, None, :] - wp[None]) ** 2).sum(2)).min(1)
    assert d.max() < np.sqrt((np.diff(np.vstack([wp, wp[:1]]), axis=0) ** 2).sum(1)).max()      # on the track: nearer to a waypoint than a segment is long
    assert np.array_equal(car, pkg.scenarios.track_starts(512, params, waypoints, seed=1))


def test_short_call_forms_of_the_core(golden_dir):
    """tests/cpp/drive_call_forms_test.cpp: mpc::drive_plant and mpc::drive_step_instance without plant values / substep counts /
    model values are the full form on the default column, bit for bit (a stand-alone program, no contraction)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "carnd-mpc-project_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drive_call_forms_test")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(root, "include"), "-I" + csrc,
                               os.path.join(root, "tests", "cpp", "drive_call_forms_test.cpp"), os.path.join(csrc, "mpc_params.cpp"), "-lm", "-o", exe])
        p = subprocess.run([exe, os.path.join(golden_dir, "config-fast.json")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "bad 0" in p.stdout, (p.stdout, p.stderr[-2000:])
