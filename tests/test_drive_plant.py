"""Track driving with per-car plant values (the mpc_drive_*_plant entry points of include/mpc_amd_drive.h), checked without a GPU: the
declarations and the host-only ABI; the CPU build of the plant loop (tests/drive_twin) -- its plant against the substep of the
header written once more in long double, the default column against the build without a plant array, the loop against its own
records, a side drift on the lake track, unusable columns -- and a stand-alone program around it under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import drive_helpers as D
import drive_latency_helpers as DL
import drive_plant_helpers as DP
from helpers import ROOT
from run_model_helpers import uniform_model

DRIVE_FORMS = ("mpc_drive_batch_device", "mpc_drive_batch_device_fused", "mpc_drive_batch_host")


@pytest.fixture(scope="module")
def twin():
    return D.load_drive_twin()


def _declared(header, name):
    found = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, re.M | re.S)
    assert found, name
    return [" ".join(q.split()) for q in found.group(1).split(",")]


def test_declarations_and_host_only_abi(pkg, golden_dir):
    """Each _plant form is its _horizon form plus `const double *plant` behind `latency`; exported, bound; a NULL handle gives -1, also
    with a plant array.  mpc_drive_plant_default: {Lf, 1, 0, 6, 50, 0} without a device, NULL arguments refused.  The constants of the
    header as a C compiler sees them; the ABI version and MpcDriveOpts stay."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    inc = os.path.join(_abi.ROOT, "include")
    drive_h = open(os.path.join(inc, "mpc_amd_drive.h")).read()
    for f in DRIVE_FORMS:
        name, base = f + "_plant", _declared(drive_h, f + "_horizon")
        assert name in _abi.DRIVE_EXPORTS and hasattr(lib, name), name
        got = _declared(drive_h, name)
        at = base.index("const double *latency")
        assert got == base[:at + 1] + ["const double *plant"] + base[at + 1:], (name, base, got)
        base_types, bound = getattr(lib, f + "_horizon").argtypes, getattr(lib, name).argtypes
        assert bound is not None and list(bound) == list(base_types[:at + 1]) + [C.c_void_p] + list(base_types[at + 1:]), name
        args = [None if "*" in q else (0.0 if q.startswith("double ") else 0) for q in got]
        assert getattr(lib, name)(*args) == -1 and b"NULL handle" in lib.mpc_last_error(), name
        a = np.zeros((6, 1))
        args[at + 1] = a.ctypes.data
        assert getattr(lib, name)(*args) == -1 and b"NULL handle" in lib.mpc_last_error(), name
    assert not any("telemetry" in n and "plant" in n for n in _abi.DRIVE_EXPORTS)      # the handler reads nothing of the plant
    assert (_abi.NPLANT, _abi.PLANT_LF, _abi.PLANT_STEER_GAIN, _abi.PLANT_STEER_BIAS, _abi.PLANT_ACCEL_GAIN, _abi.PLANT_DRAG_SPEED,
            _abi.PLANT_DRIFT) == (6, 0, 1, 2, 3, 4, 5)
    assert lib.mpc_abi_version() == 5
    # mpc_drive_plant_default
    assert _declared(drive_h, "mpc_drive_plant_default") == ["const MpcParams *p", "double *col6"]
    for cfg in ("config-fast.json", "config-stable.json"):
        params = pkg.params_from_json(os.path.join(golden_dir, cfg))
        col = np.full(7, D.SENTINEL)
        assert lib.mpc_drive_plant_default(C.byref(params), col.ctypes.data) == 0
        assert col.tolist() == [params.Lf, 1.0, 0.0, 6.0, 50.0, 0.0, D.SENTINEL]
        assert np.array_equal(pkg.drive_plant_default(params), col[:6])
    col = np.full(6, D.SENTINEL)
    assert lib.mpc_drive_plant_default(None, col.ctypes.data) == -1 and b"NULL" in lib.mpc_last_error() and (col == D.SENTINEL).all()
    assert lib.mpc_drive_plant_default(C.byref(params), None) == -1 and b"NULL" in lib.mpc_last_error()
    model = uniform_model(params, 5); model[1] = [1.0, 2.0, 3.0, 4.0, 5.0]
    a = pkg.drive_plant_default(params, 5, model)
    assert a.shape == (6, 5) and a.flags.c_contiguous and np.array_equal(a[0], model[1]) and np.array_equal(a[1:], np.repeat([[1.0], [0.0], [6.0], [50.0], [0.0]], 5, 1))
    assert np.array_equal(pkg.drive_plant_default(params, 5)[0], np.full(5, params.Lf))
    src = ('#include <stdio.h>\n#include "mpc_amd.h"\nint main(){printf("%d %d %d %d %d %d %d %d\\n", (int)sizeof(MpcDriveOpts), MPC_NPLANT, MPC_PLANT_LF, '
           'MPC_PLANT_STEER_GAIN, MPC_PLANT_STEER_BIAS, MPC_PLANT_ACCEL_GAIN, MPC_PLANT_DRAG_SPEED, MPC_PLANT_DRIFT);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", inc, "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        assert [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()] == [C.sizeof(_abi.MpcDriveOpts), 6, 0, 1, 2, 3, 4, 5] == [48, 6, 0, 1, 2, 3, 4, 5]


def _plant_cars(B):
    """the draws of tests/test_drive.py::test_plant"""
    g = np.random.default_rng(11)
    car = np.stack([g.uniform(-200, 200, B), g.uniform(-200, 200, B), g.uniform(-np.pi, np.pi, B), g.uniform(10, 80, B), g.uniform(-0.4, 0.4, B),
                    g.uniform(-1, 1, B)])
    cmd = np.stack([g.uniform(-1, 1, B), g.uniform(-1, 1, B)])
    cmd[0, 3] = np.nan; cmd[1, 4] = np.inf; cmd[:, 5] = np.nan      # a reply that is not finite keeps the old command
    return car, cmd


@pytest.mark.parametrize("sub_old,sub_new", [(10, 2), (0, 10), (3, 0)])
def test_plant_against_the_long_double_substep(pkg, twin, golden_dir, sub_old, sub_new):
    """256 cars (the draws of tests/test_drive.py::test_plant) with the columns of draw_plant against the substep of the header written in
    np.longdouble, h = 0.01.  The bound per row: 8 x substeps x 1 ulp of max(1, |value|) -- at most eight rounded operations feed a row in
    one substep (x and y: dist, sin, cos, w * h, two products, two sums), test_plant's rule with 8 for its 4.  The bound is attainable:
    the same formula in plain np.float64 stays inside it against the same reference (asserted; below 1.0 of substeps x ulp here)."""
    B, h = 256, 0.01
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps / 1000, "the reference needs a long double wider than double"
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    car, cmd = _plant_cars(B)
    plant = DP.draw_plant(B)
    model = uniform_model(params, B)
    got, ok = DP.twin_plant(twin, params, car, cmd, model, plant, sub_old, sub_new, h)
    assert ok.all()
    ref = DP.reference_plant(car, cmd, params.max_steering, plant, sub_old, sub_new, h)
    ref64 = ref.astype(np.float64)
    ulp = (sub_old + sub_new) * np.spacing(np.maximum(1.0, np.abs(ref64)))
    bound = 8 * ulp
    err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
    plain = DP.reference_plant(car, cmd, params.max_steering, plant, sub_old, sub_new, h, dtype=np.float64)
    err_plain = np.abs((plain.astype(np.longdouble) - ref).astype(np.float64))
    print("plant (%d, %d): max error / bound per row %s; plain float64 / bound %s" % (sub_old, sub_new, (err / bound).max(1), (err_plain / bound).max(1)))
    assert (err_plain <= bound).all()
    assert (err <= bound).all()
    keep = [3, 4, 5]
    assert np.array_equal(got[4:, keep], car[4:, keep])              # the old command is still in force
    rest = np.setdiff1d(np.arange(B), keep)
    assert np.array_equal(got[4, rest], cmd[0, rest] * params.max_steering) and np.array_equal(got[5, rest], cmd[1, rest])
    # the column reaches the plant: every row that it feeds differs from the plant without one
    none = D.twin_plant(D.load_drive_twin(), params, car, cmd, sub_old, sub_new, h)
    assert (got[:4] != none[:4]).mean() > 0.9


def test_a_standing_car_on_a_zero_coordinate(pkg, twin, golden_dir):
    """The sign of a coordinate that is exactly zero.  Every form moves the car with x = x - (w * h) * sin(psi), y = y + (w * h) * cos(psi)
    behind the expressions from before the plant columns, w = 0 without a plant array, so a car that stands (speed, steering, throttle 0)
    on -0.0 may be put on +0.0 where those expressions alone left it.  Pinned here: no plant array and the default column give the same
    bytes, and the signs are those of the header's statements in IEEE arithmetic (a fused multiply-add of an exact zero product has
    them too)."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), N=10)
    psi = np.array([0.3, -0.3, 2.0, -2.0, 0.0, np.pi] * 4)
    B = len(psi)
    car = np.zeros((6, B)); car[2] = psi
    car[0] = np.repeat([0.0, -0.0, 0.0, -0.0], 6); car[1] = np.repeat([0.0, 0.0, -0.0, -0.0], 6)
    cmd, h = np.zeros((2, B)), 0.01
    none = D.twin_plant(twin, params, car, cmd, 1, 1, h)
    col, ok = DP.twin_plant(twin, params, car, cmd, uniform_model(params, B), pkg.drive_plant_default(params, B), 1, 1, h)
    assert ok.all() and none.tobytes() == col.tobytes()
    x, y = car[0].copy(), car[1].copy()
    for _ in range(2):
        x = (x + (0.0 * h) * np.cos(psi)) - (0.0 * h) * np.sin(psi)
        y = (y + (0.0 * h) * np.sin(psi)) + (0.0 * h) * np.cos(psi)
    assert (none[:2] == 0.0).all() and np.array_equal(np.signbit(none[0]), np.signbit(x)) and np.array_equal(np.signbit(none[1]), np.signbit(y))
    assert np.signbit(car[:2]).sum() > np.signbit(none[:2]).sum() > 0          # some -0.0 became +0.0, some stayed
    assert np.array_equal(none[2:], car[2:])


@pytest.fixture(scope="module")
def setup16(pkg, golden_dir, waypoints):
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), N=10)
    return params, pkg.scenarios.track_starts(16, params, waypoints, seed=3), uniform_model(params, 16), DL.draw_latency(16)


@pytest.mark.parametrize("warm", [0, 1])
def test_default_column_is_the_latency_twin(pkg, twin, setup16, waypoints, warm):
    """the default column (its Lf row: the car's own Lf, here a model array with different Lf values): bitwise the
    tests/drive_twin loop on 16 cars x 8 steps"""
    params, car, model, lat = setup16
    model = model.copy(); model[1] = np.linspace(2.2, 3.2, 16)
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    a = DP.twin_drive_plant(twin, params, waypoints, car, model, lat, pkg.drive_plant_default(params, 16, model), 8, opts, wopts)
    b = DL.twin_drive_latency(D.load_drive_twin(), params, waypoints, car, model, lat, 8, opts, wopts)
    DP.same(a, b)
    assert np.array_equal(a["handler_status"], a["hist"][:, D.REC_STATUS].astype(np.int32))


@pytest.mark.parametrize("warm", [0, 1])
def test_the_loop_is_its_records(pkg, twin, setup16, waypoints, warm):
    """a mixed plant array: the car of step t + 1 is the twin's plant on the car and reply of step t, bitwise, with the car's own column
    and substep counts; rows 4 and 5 stay the commanded values"""
    params, car, model, lat = setup16
    plant = DP.draw_plant(16)
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    res = DP.twin_drive_plant(twin, params, waypoints, car, model, lat, plant, 8, opts, wopts)
    hist = res["hist"]
    assert np.isfinite(hist).all()
    for t in range(8):
        nxt = hist[t + 1, :6] if t < 7 else res["car"]
        for i in range(16):
            ref, ok = DP.twin_plant(twin, params, hist[t, :6, i:i + 1], hist[t, D.REC_CMD:D.REC_CMD + 2, i:i + 1], model[:, i:i + 1], plant[:, i:i + 1],
                                    int(lat[DL.SUB_OLD, i]), int(lat[DL.SUB_NEW, i]), opts.h)
            assert ok.all() and np.array_equal(ref[:, 0], nxt[:, i]), (t, i)
        assert np.array_equal(nxt[4], hist[t, D.REC_CMD] * params.max_steering) and np.array_equal(nxt[5], hist[t, D.REC_CMD + 1])
    D.check_summary(res, len(waypoints), opts.cte_limit)


def test_side_drift_on_the_lake_track(pkg, twin, golden_dir, waypoints):
    """config-fast, 8 cars x 40 messages: with w = +1 the mean of cte0 over the last 20 messages is not zero, with w = -1 it has the
    opposite sign, and the w = 0 column gives the _latency results bitwise."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    B = 8
    car = pkg.scenarios.track_starts(B, params, waypoints, seed=3)
    model = uniform_model(params, B)
    opts, wopts = pkg.drive_opts_default(params, warm_start=1), pkg.warm_opts_default()
    lat = DL.uniform_latency(B, DL.handle_comp(params), opts.sub_old, opts.sub_new)
    col = pkg.drive_plant_default(params)
    res = {}
    for w in (1.0, 0.0, -1.0):
        c = col.copy(); c[DP.DRIFT] = w
        res[w] = DP.twin_drive_plant(twin, params, waypoints, car, model, lat, DP.uniform_plant(B, c), 40, opts, wopts)
    mean = {w: r["hist"][20:, D.REC_CTE].mean() for w, r in res.items()}
    print("mean cte0 over the last 20 messages: w = +1 %.4f, w = 0 %.4f, w = -1 %.4f" % (mean[1.0], mean[0.0], mean[-1.0]))
    assert mean[1.0] != 0.0 and mean[-1.0] != 0.0 and np.sign(mean[1.0]) == -np.sign(mean[-1.0])
    DP.same(res[0.0], DL.twin_drive_latency(D.load_drive_twin(), params, waypoints, car, model, lat, 40, opts, wopts))


@pytest.mark.parametrize("warm", [0, 1])
def test_unusable_columns(pkg, twin, setup16, waypoints, warm):
    """Not-a-number and infinity in each row, Lf_p = 0 and -1, d = 0 (15 columns, in cars 1 .. 15 of 16): the car is moved with the
    default column, every step that the handler ended SUCCESS or ACCEPTABLE is INFEASIBLE in hist row 10, summary row 7 and the folded
    status, nothing is not-a-number, the iterations and every other car are unchanged -- and in a warm call the car's next step is
    still warm-started, because the handler's own status is not touched: its replies are those of the clean run."""
    params, car, model, lat = setup16
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    default = pkg.drive_plant_default(params, 16)
    clean = DP.twin_drive_plant(twin, params, waypoints, car, model, lat, default, 8, opts, wopts)
    cols = DP.unusable_columns(default[:, 0])
    assert len(cols) == 15
    dirty = default.copy()
    for i, (_, c) in enumerate(cols):
        dirty[:, i + 1] = c
    _, ok = DP.twin_plant(twin, params, car, np.zeros((2, 16)), model, dirty, 1, 1, opts.h)
    assert ok.tolist() == [1] + [0] * 15
    res = DP.twin_drive_plant(twin, params, waypoints, car, model, lat, dirty, 8, opts, wopts)
    bad = np.arange(1, 16)
    hs = res["handler_status"]
    assert np.array_equal(hs, clean["handler_status"]) and (hs[:, bad] == 0).sum() > 100       # the handler is untouched; it succeeded there
    want = DP.expected_status(hs[:, bad])
    assert np.array_equal(res["hist"][:, D.REC_STATUS][:, bad].astype(np.int32), want) and (want != 0).all()
    assert (res["summary"][7, bad] == 8).all() and np.array_equal(res["status"][bad], want.max(0))
    for k in ("car", "summary", "hist"):
        assert np.isfinite(res[k]).all(), k
    assert np.array_equal(res["iters"], clean["iters"]) and np.array_equal(res["hist"][:, D.REC_ITERS], clean["hist"][:, D.REC_ITERS])
    DP.same(res, clean, cars=[0])
    # moved with the default column, and started warm where the clean run started warm: apart from the status rows, the clean run's bits
    other = [r for r in range(D.REC) if r != D.REC_STATUS]
    assert np.array_equal(res["hist"][:, other], clean["hist"][:, other]) and np.array_equal(res["car"], clean["car"])
    assert np.array_equal(res["summary"][:7], clean["summary"][:7])
    if warm:
        cold = DP.twin_drive_plant(twin, params, waypoints, car, model, lat, default, 8, pkg.drive_opts_default(params, warm_start=0), wopts)
        assert not np.array_equal(cold["hist"][1:, D.REC_ITERS], clean["hist"][1:, D.REC_ITERS])      # (a warm step is not the cold step)


def test_plant_loop_on_garbage_under_asan_ubsan(golden_dir):
    """tests/cpp/drive_plant_sanitize.cpp: a stand-alone program around the CPU build and mpc_params.cpp, compiled with
    -fsanitize=address,undefined and run directly; its input includes the unusable columns."""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "carnd-mpc-project_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drive_plant_sanitize")
        subprocess.check_call(["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "cpp", "drive_plant_sanitize.cpp"),
                                                                   os.path.join(ROOT, "tests", "drive_twin", "drive_twin.cpp"),
                                                                   os.path.join(ROOT, "carnd-mpc-project_amd", "csrc", "mpc_params.cpp"), "-lm", "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, os.path.join(golden_dir, "config-fast.json")], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rows = re.findall(r"^warm (\d) status((?: \d+){12})$", p.stdout, re.M)
    assert [r[0] for r in rows] == ["0", "1"] and "bad 0" in p.stdout, p.stdout
    for _, line in rows:
        st = [int(v) for v in line.split()]
        assert st[0] == 0 and st[11] == 0 and all(st[1:11]), p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
