"""Track driving and the telemetry handler with a per-car horizon (the mpc_drive_*_horizon and mpc_telemetry_batch_*_horizon entry
points of include/mpc_amd_drive.h), checked without a GPU: the declarations; the CPU build of the horizon loop
(tests/drive_twin) -- with every horizon the handle's N against the latency twin, a mixed batch against the latency twin run with
MpcParams.N = horizon[i], every recorded solve of the mixed batch against the oracle with N = horizon[i], unusable horizons, the summary
rows -- and a stand-alone program around it under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import drive_helpers as D
import drive_horizon_helpers as DH
import drive_latency_helpers as DL
from helpers import ROOT
from horizon_helpers import LOOP_HORIZONS, with_N
from model_helpers import draw_rows
from run_model_helpers import uniform_model

DRIVE_FORMS = ("mpc_drive_batch_device", "mpc_drive_batch_device_fused", "mpc_drive_batch_host")
TELEMETRY_FORMS = ("mpc_telemetry_batch_device", "mpc_telemetry_batch_host")
B16, STEPS = 16, 8


@pytest.fixture(scope="module")
def twin():
    return D.load_drive_twin()


def _declared(header, name):
    found = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, re.M | re.S)
    assert found, name
    return [" ".join(q.split()) for q in found.group(1).split(",")]


def test_declarations(pkg):
    """Each of the five forms is its _latency form plus `const int32_t *horizon` behind `model`; exported, bound; a NULL handle gives -1
    with and without a horizon; the ABI version stays 5 and _abi.HORIZON_EXPORTS its seven names."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    drive_h = open(os.path.join(_abi.ROOT, "include", "mpc_amd_drive.h")).read()
    for f in DRIVE_FORMS + TELEMETRY_FORMS:
        name, base_name = f + "_horizon", f + "_latency"
        assert name in _abi.DRIVE_EXPORTS and name not in _abi.HORIZON_EXPORTS and hasattr(lib, name), name
        base, got = _declared(drive_h, base_name), _declared(drive_h, name)
        at = base.index("const double *model")
        assert got == base[:at + 1] + ["const int32_t *horizon"] + base[at + 1:], (name, base, got)
        base_types, bound = getattr(lib, base_name).argtypes, getattr(lib, name).argtypes
        assert bound is not None and list(bound) == list(base_types[:at + 1]) + [C.c_void_p] + list(base_types[at + 1:]), name
        args = [None if "*" in q else (0.0 if q.startswith("double ") else 0) for q in got]
        assert getattr(lib, name)(*args) == -1 and b"NULL handle" in lib.mpc_last_error(), name
        hz = np.full(1, 5, dtype=np.int32)                       # ... also with a horizon and nothing else
        args[at + 1] = hz.ctypes.data
        assert getattr(lib, name)(*args) == -1 and b"NULL handle" in lib.mpc_last_error(), name
    assert lib.mpc_abi_version() == 5
    assert len(_abi.HORIZON_EXPORTS) == 7 and all(n.startswith(("mpc_solve_", "mpc_rollout_")) for n in _abi.HORIZON_EXPORTS)
    for name, text in (("mpc_amd_drive.h", drive_h), ("mpc_amd_horizon.h", open(os.path.join(_abi.ROOT, "include", "mpc_amd_horizon.h")).read())):
        assert "no _horizon form" not in text and "have none, deliberately" not in text, name


def _cars(pkg, params, waypoints):
    return pkg.scenarios.track_starts(B16, params, waypoints, seed=3)


@pytest.mark.parametrize("warm", [0, 1])
def test_all_horizons_N_is_the_latency_twin(pkg, twin, golden_dir, waypoints, warm):
    """horizon = all N: bitwise tests/drive_twin on the same 16 cars x 8 messages, with and without model and latency columns
    (without: the handle's own values and the call's own scalars, which is what model == NULL is in the horizon twin)."""
    params = DH.fast_params(pkg, golden_dir)
    opts, wopts = pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()
    car = _cars(pkg, params, waypoints)
    hz = np.full(B16, params.N, dtype=np.int32)
    plain_lat = DH.default_latency(params, opts, B16)
    for model, lat in ((None, None), (draw_rows(params, B16, seed=9), DL.draw_latency(B16))):
        ref = DL.twin_drive_latency(twin, params, waypoints, car, model if model is not None else uniform_model(params, B16),
                                    lat if lat is not None else plain_lat, STEPS, opts, wopts)
        got = DH.twin_drive_horizon(twin, params, waypoints, car, hz, STEPS, opts, wopts, model=model, latency=lat)
        DH.same(got, ref)
        if model is None:        # ... and a model array of the handle's own values is model == NULL
            DH.same(DH.twin_drive_horizon(twin, params, waypoints, car, hz, STEPS, opts, wopts, model=uniform_model(params, B16)), ref)


@pytest.fixture(scope="module")
def mixed(pkg, twin, golden_dir, waypoints):
    """16 cars, horizon (3, 4, 5, 7, 10)[i % 5] on an N = 10 handle, 8 messages, config-fast, default drive options, cold and warm:
    computed once."""
    params = DH.fast_params(pkg, golden_dir)
    car = _cars(pkg, params, waypoints)
    hz = DH.mixed_horizons(B16)
    out = {}
    for warm in (0, 1):
        opts = pkg.drive_opts_default(params, warm_start=warm)
        out[warm] = (params, opts, car, hz, DH.twin_drive_horizon(twin, params, waypoints, car, hz, STEPS, opts, pkg.warm_opts_default()))
    return out


@pytest.mark.parametrize("warm", [0, 1])
def test_a_mixed_batch_is_its_uniform_parts(pkg, twin, waypoints, mixed, warm):
    """Car i is bitwise car i of the latency twin run with MpcParams.N = horizon[i]; and the horizon reaches the solve: the cars of the
    other groups differ."""
    params, opts, car, hz, res = mixed[warm]
    assert sorted(set(hz.tolist())) == list(LOOP_HORIZONS)
    for n in LOOP_HORIZONS:
        q = with_N(params, n)
        ref = DL.twin_drive_latency(twin, q, waypoints, car, uniform_model(q, B16), DH.default_latency(q, opts, B16), STEPS, opts,
                                    pkg.warm_opts_default())
        DH.same(res, ref, cars=np.nonzero(hz == n)[0])
        others = np.nonzero(hz != n)[0]
        assert not np.array_equal(res["hist"][:, D.REC_CMD][:, others], ref["hist"][:, D.REC_CMD][:, others])


@pytest.mark.parametrize("warm", [0, 1])
def test_mixed_batch_against_the_oracle(mixed, waypoints, warm):
    """Every recorded (car, window) of the mixed batch against oracle_lib.telemetry_handler on a config loaded with N = horizon[i]: the
    same status, steer within TOL_STEER / max_steering, throttle within drive_helpers.TOL_THROTTLE; 128 of 128 pairs."""
    params, opts, car, hz, res = mixed[warm]
    d_steer, d_thr, pairs = DH.oracle_check_steps_horizon("config-fast.json", params, hz, waypoints, res["hist"], opts.extra_latency)
    print("warm %d: %d pairs, max |d steer| %.3g rad, |d throttle| %.3g; iterations per solve %.2f" % (
        warm, pairs, d_steer, d_thr, res["hist"][:, D.REC_ITERS].mean()))
    assert pairs == B16 * STEPS
    assert np.isfinite(res["hist"]).all() and (res["hist"][:, D.REC_STATUS] == 0).all()


@pytest.mark.parametrize("warm", [0, 1])
def test_unusable_horizons(pkg, twin, waypoints, mixed, warm):
    """2, 0, -1 and N + 1 at four cars: INFEASIBLE at every step, summary row 7 = steps, no not-a-number in car, summary or hist; every
    other car bitwise the batch without the defect."""
    params, opts, car, hz, clean = mixed[warm]
    bad = [2, 7, 11, 14]
    dirty = DH.unusable(hz, bad, params.N)
    assert dirty[bad].tolist() == [2, 0, -1, 11]
    res = DH.twin_drive_horizon(twin, params, waypoints, car, dirty, STEPS, opts, pkg.warm_opts_default())
    DH.check_unusable(res, clean, bad, STEPS)
    D.check_summary(res, len(waypoints), opts.cte_limit)


@pytest.mark.parametrize("warm", [0, 1])
def test_summary_rows(mixed, waypoints, warm):
    """the summary rows recomputed from the records"""
    params, opts, car, hz, res = mixed[warm]
    D.check_summary(res, len(waypoints), opts.cte_limit)
    hist = res["hist"]
    assert (hist[1:, 4] == hist[:-1, D.REC_CMD] * params.max_steering).all() and (hist[1:, 5] == hist[:-1, D.REC_CMD + 1]).all()


def test_horizon_loop_under_asan_ubsan(pkg, golden_dir, waypoints):
    """tests/cpp/drive_horizon_sanitize.cpp: a stand-alone program around the CPU build, compiled with -fsanitize=address,undefined and
    run directly, on the mixed batch and on the unusable horizons.  Nothing is loaded into Python under a sanitizer."""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "carnd-mpc-project_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    params = DH.fast_params(pkg, golden_dir)
    car = _cars(pkg, params, waypoints)
    tx, ty = D.track_of(waypoints)
    with tempfile.TemporaryDirectory() as d:
        exe, data = os.path.join(d, "drive_horizon_sanitize"), os.path.join(d, "cars.txt")
        with open(data, "w") as f:
            f.write("%d %d\n" % (len(tx), B16))
            for row in [tx, ty] + list(car):
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
        subprocess.check_call(["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "cpp", "drive_horizon_sanitize.cpp"),
                                                                   os.path.join(ROOT, "tests", "drive_twin", "drive_twin.cpp"),
                                                                   os.path.join(ROOT, "carnd-mpc-project_amd", "csrc", "mpc_params.cpp"), "-lm", "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, os.path.join(golden_dir, "config-fast.json"), data], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rows = re.findall(r"^warm (\d) (mixed|dirty)((?: \d+){16})$", p.stdout, re.M)
    assert [(r[0], r[1]) for r in rows] == [("0", "mixed"), ("0", "dirty"), ("1", "mixed"), ("1", "dirty")] and "bad 0" in p.stdout, p.stdout
    for _, kind, line in rows:
        st = [int(v) for v in line.split()]
        assert [i for i, v in enumerate(st) if v != 0] == ([] if kind == "mixed" else [2, 7, 11, 14]), p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
