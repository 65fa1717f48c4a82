"""Track driving with per-car model values (the mpc_drive_*_model entry points of include/mpc_amd_drive.h), checked without a GPU:
the declarations; the CPU build of the model loop (tests/drive_twin) -- its plant against the composition of the oracle's
Vehicle::move with every car's own Lf and max_steering and against the model-free build, its loop against the oracle's telemetry
handler with a per-car Config on every recorded step, unusable columns -- and a stand-alone program around it under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import drive_helpers as D
import drive_model_helpers as DM
from helpers import ROOT
from model_helpers import INFEASIBLE, draw_rows
from run_model_helpers import uniform_model

MODEL_FORMS = ("mpc_drive_batch_device_model", "mpc_drive_batch_device_fused_model", "mpc_drive_batch_host_model")


@pytest.fixture(scope="module")
def twin():
    return D.load_drive_twin()


def test_declarations(pkg, golden_dir):
    """Declared with `model` directly behind `weights`, exported, bound; a NULL handle gives -1; the ABI version and MpcDriveOpts stay."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    header = open(os.path.join(_abi.ROOT, "include", "mpc_amd_drive.h")).read()
    for name in MODEL_FORMS:
        assert name in _abi.DRIVE_EXPORTS and hasattr(lib, name), name
        plain = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name[:-len("_model")], header, re.M | re.S).group(1)
        model = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, re.M | re.S).group(1)
        norm = lambda s: [" ".join(q.split()) for q in s.split(",")]
        a, b = norm(plain), norm(model)
        at = a.index("const double *weights")
        assert b == a[:at + 1] + ["const double *model"] + a[at + 1:], (name, a, b)
        base, bound = getattr(lib, name[:-len("_model")]).argtypes, getattr(lib, name).argtypes
        assert bound is not None and list(bound) == list(base[:at + 1]) + [C.c_void_p] + list(base[at + 1:]), name
        args = [None if "*" in q else 0 for q in b]
        assert getattr(lib, name)(*args) == -1 and b"NULL handle" in lib.mpc_last_error(), name
        # ... also with a model array and nothing else
        m = np.zeros((6, 1))
        args[at + 1] = m.ctypes.data
        assert getattr(lib, name)(*args) == -1 and b"NULL handle" in lib.mpc_last_error(), name
    assert lib.mpc_abi_version() == 5
    src = '#include <stdio.h>\n#include "mpc_amd.h"\nint main(){printf("%d\\n", (int)sizeof(MpcDriveOpts));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(_abi.ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        assert int(subprocess.check_output([os.path.join(d, "t")])) == C.sizeof(_abi.MpcDriveOpts) == 48


def _plant_cars(B):
    g = np.random.default_rng(11)
    car = np.stack([g.uniform(-200, 200, B), g.uniform(-200, 200, B), g.uniform(-np.pi, np.pi, B), g.uniform(10, 80, B), g.uniform(-0.4, 0.4, B),
                    g.uniform(-1, 1, B)])
    cmd = np.stack([g.uniform(-1, 1, B), g.uniform(-1, 1, B)])
    cmd[0, 3] = np.nan; cmd[1, 4] = np.inf; cmd[:, 5] = np.nan      # a reply that is not finite keeps the old command
    return car, cmd


@pytest.mark.parametrize("sub_old,sub_new", [(10, 2), (0, 10), (3, 0)])
def test_plant_with_a_column(pkg, twin, golden_dir, sub_old, sub_new):
    """256 cars with the columns of draw_rows against the composition of O.vehicle_move with each car's own Lf and the reply scaled by
    its own max_steering.  The bound is that of tests/test_drive.py::test_plant, for the reason stated there: 4 x substeps x 1 ulp of
    max(1, |value|) -- a column changes the operands of the operations, not their number.  With uniform_model the plant is bitwise the
    model-free build's: the same doubles in the same expressions."""
    B, h = 256, 0.01
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    model = draw_rows(params, B)
    car, cmd = _plant_cars(B)
    got = DM.twin_plant_model(twin, params, car, cmd, model, sub_old, sub_new, h)
    ref = DM.oracle_plant_model("config-fast.json", car, cmd, model, sub_old, sub_new, h)
    bound = 4 * (sub_old + sub_new) * np.spacing(np.maximum(1.0, np.abs(ref)))
    err = np.abs(got - ref)
    print("plant with a column (%d, %d): max error / bound per row %s" % (sub_old, sub_new, (err / bound).max(1)))
    assert (err <= bound).all()
    keep = [3, 4, 5]
    assert np.array_equal(got[4:, keep], car[4:, keep])
    ok = np.setdiff1d(np.arange(B), keep)
    assert np.array_equal(got[4, ok], cmd[0, ok] * model[2, ok]) and np.array_equal(got[5, ok], cmd[1, ok])
    # the columns reach the plant: another Lf, another heading
    plain = D.twin_plant(D.load_drive_twin(), params, car, cmd, sub_old, sub_new, h)
    assert not np.array_equal(got[2], plain[2])
    assert np.array_equal(DM.twin_plant_model(twin, params, car, cmd, uniform_model(params, B), sub_old, sub_new, h), plain)


@pytest.fixture(scope="module")
def loops(pkg, twin, golden_dir, waypoints):
    """16 cars x 8 messages, N = 10, the columns draw_rows(seed 9), config-fast and config-stable, cold and warm: computed once."""
    out = {}
    for cfgname in ("config-fast.json", "config-stable.json"):
        params = pkg.params_from_json(os.path.join(golden_dir, cfgname), N=10)
        car = pkg.scenarios.track_starts(16, params, waypoints, seed=3)
        model = draw_rows(params, 16, seed=9)
        for warm in (0, 1):
            opts = pkg.drive_opts_default(params, warm_start=warm)
            out[cfgname, warm] = (params, opts, model, DM.twin_drive_model(twin, params, waypoints, car, model, 8, opts, pkg.warm_opts_default()))
    return out


@pytest.mark.parametrize("cfgname", ["config-fast.json", "config-stable.json"])
@pytest.mark.parametrize("warm", [0, 1])
def test_loop_against_the_oracle(loops, waypoints, cfgname, warm):
    """Every recorded (car, window) against the oracle's telemetry handler with the car's own Config: 128 of 128 pairs, all SUCCESS.
    The records are the loop: the car of step t + 1 carries cmd_steer x max_steering_i in row 4; the summary follows from them."""
    params, opts, model, res = loops[cfgname, warm]
    d_steer, d_thr, pairs = DM.oracle_check_steps_model(cfgname, {"N": 10}, model, waypoints, res["hist"], opts.extra_latency)
    print("%s warm %d: %d pairs, max |d steer| %.3g rad, |d throttle| %.3g; iterations per solve %.2f" % (
        cfgname, warm, pairs, d_steer, d_thr, res["hist"][:, D.REC_ITERS].mean()))
    assert pairs == 128
    hist = res["hist"]
    assert np.isfinite(hist).all() and (hist[:, D.REC_K] == np.round(hist[:, D.REC_K])).all()
    assert (hist[1:, 4] == hist[:-1, D.REC_CMD] * model[2][None, :]).all() and (hist[1:, 5] == hist[:-1, D.REC_CMD + 1]).all()
    D.check_summary(res, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("warm", [0, 1])
def test_uniform_model_is_the_model_free_loop(pkg, twin, loops, waypoints, warm):
    """every column the handle's own values: bitwise the CPU build without a model array"""
    params, opts, _, _ = loops["config-fast.json", warm]
    car = pkg.scenarios.track_starts(16, params, waypoints, seed=3)
    a = DM.twin_drive_model(twin, params, waypoints, car, uniform_model(params, 16), 4, opts, pkg.warm_opts_default())
    b = D.twin_drive(D.load_drive_twin(), params, waypoints, car, 4, opts, pkg.warm_opts_default())
    for k in ("car", "summary", "hist", "status", "iters"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("warm", [0, 1])
def test_unusable_columns(pkg, twin, loops, waypoints, warm):
    """NaN, dt = 0, Lf = -1 and max_acceleration = 0 in single cars of the 16: INFEASIBLE at every step with finite rows -- the
    handle's values take the column's place around the solve and in the plant --, and every other car bitwise the batch without the
    defect."""
    params, opts, model, clean = loops["config-fast.json", warm]
    car = pkg.scenarios.track_starts(16, params, waypoints, seed=3)
    dirty = model.copy()
    bad = [2, 7, 11, 14]
    dirty[5, 2] = np.nan; dirty[0, 7] = 0.0; dirty[1, 11] = -1.0; dirty[3, 14] = 0.0
    res = DM.twin_drive_model(twin, params, waypoints, car, dirty, 8, opts, pkg.warm_opts_default())
    assert (res["hist"][:, D.REC_STATUS][:, bad] == INFEASIBLE).all() and (res["status"][bad] == INFEASIBLE).all()
    assert (res["summary"][7, bad] == 8).all()
    for k in ("car", "summary", "hist"):
        assert np.isfinite(res[k][..., bad]).all(), k
    good = np.setdiff1d(np.arange(16), bad)
    for k in ("car", "summary", "hist", "status", "iters"):
        assert np.array_equal(res[k][..., good], clean[k][..., good]), k
    # the plant of such a car runs on the handle's values: its first step is the model-free plant on its start and reply
    h0 = res["hist"][0]
    nxt = D.twin_plant(D.load_drive_twin(), params, h0[:6, bad], h0[D.REC_CMD:D.REC_CMD + 2, bad], opts.sub_old, opts.sub_new, opts.h)
    assert np.array_equal(nxt, res["hist"][1, :6, bad].T)


def test_model_loop_on_garbage_under_asan_ubsan(golden_dir):
    """tests/cpp/drive_model_sanitize.cpp: a stand-alone program around the CPU build, compiled with -fsanitize=address,undefined and
    run directly."""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "carnd-mpc-project_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drive_model_sanitize")
        subprocess.check_call(["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "cpp", "drive_model_sanitize.cpp"),
                                                                   os.path.join(ROOT, "tests", "drive_twin", "drive_twin.cpp"),
                                                                   os.path.join(ROOT, "carnd-mpc-project_amd", "csrc", "mpc_params.cpp"), "-lm", "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, os.path.join(golden_dir, "config-fast.json")], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rows = re.findall(r"^warm (\d) status((?: \d+){8})$", p.stdout, re.M)
    assert [r[0] for r in rows] == ["0", "1"] and "bad 0" in p.stdout, p.stdout
    for _, line in rows:
        st = [int(v) for v in line.split()]
        assert st[0] == 0 and st[7] == 0 and all(st[1:4]) and st[4:7] == [INFEASIBLE] * 3, p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
