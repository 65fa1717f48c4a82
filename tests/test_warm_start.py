"""Warm start of the device solver (include/mpc_amd.h, "warm start"), checked without a GPU: the CPU build tests/host_twin (mpc_twin_solve) calls the
same Solver::warm_point / begin_warm / warm_store as the kernels.  The oracle's COLD solve is the yardstick throughout: a warm
solve works on the same NLP (branch outcomes and objective scaling decided at the reference's start point) from another initial
iterate."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, closed_loop_report
from warm_helpers import garbage_warm, golden_batches, load_warm_twin, twin_closed_loop, twin_warm_solve


@pytest.fixture(scope="module")
def warm_twin():
    """TEST-ONLY CPU build of the warm start (tests/host_twin, mpc_twin_solve)."""
    return load_warm_twin()


@pytest.fixture(scope="module")
def loops(pkg, warm_twin, golden_dir, waypoints):
    """The closed loops of test_closed_loops_every_solve_against_the_oracle_cpu_build (96 cars x 25 steps, config-fast.json, seed
    122), cold and warm (library defaults), and the oracle's own."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    B, steps = 96, 25
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=122)
    opts = pkg.warm_opts_default()
    cold = twin_closed_loop(warm_twin, params, sc, steps, opts, warm_start=False)
    warm = twin_closed_loop(warm_twin, params, sc, steps, opts, warm_start=True)
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    _, oh, ost = O.rollout_chunk_full(("config-fast.json", {}, c(sc["state"]), c(sc["coeffs"]), c(sc["yaw_lo"]), c(sc["yaw_hi"]), steps))
    return {"cold": cold, "warm": warm, "oracle": (oh, ost)}


def test_warm_closed_loops_match_the_oracle(loops):
    hist, sst, _ = loops["warm"]
    oh, ost = loops["oracle"]
    assert (ost == 0).all()
    cl = closed_loop_report(hist, sst, oh, ost)
    print("warm closed loops vs oracle: max |d steer| %.3g rad, |d accel| %.3g, |d state| %.3g" % (cl["d_steer_rad"][3], cl["d_accel"][3], cl["d_state"][3]))
    assert cl["status_differs"] == 0 and cl["cars_on_another_local_minimum"] == 0, cl
    assert cl["d_steer_rad"][3] <= TOL_STEER and cl["d_accel"][3] <= TOL_ACCEL and cl["d_state"][3] <= TOL_TRAJ, cl


def test_warm_start_saves_iterations(loops):
    cold_it = int(loops["cold"][2][1:].sum()); warm_it = int(loops["warm"][2][1:].sum())
    n = loops["cold"][2][1:].size
    print("iterations per solve, steps 2..25: cold %.2f, warm %.2f, ratio %.3f" % (cold_it / n, warm_it / n, warm_it / cold_it))
    assert warm_it < cold_it


def test_warm_out_is_the_oracles_solution(pkg, warm_twin, golden_dir):
    opts = pkg.warm_opts_default()
    for cfgname, params, b in golden_batches(pkg, golden_dir):
        N = params.N
        assert pkg.warm_rows(N) == (N - 1) * pkg.WARM_REC
        r = twin_warm_solve(warm_twin, params, b, opts)
        assert (r["status"] == 0).all()
        cfg = O.load_config(cfgname)
        for i in range(b["state"].shape[1]):
            cfg.yaw_low, cfg.yaw_high = float(b["yaw_lo"][i]), float(b["yaw_hi"][i])
            st, _, _, _, _, sol = O.mpc_solve(cfg, b["state"][:, i], b["coeffs"][:, i], want_sol=True)
            assert st == 0
            v = pkg.warm_to_vars(r["warm"][:, i], b["state"][:, i], N)
            assert v.shape == sol.shape == (8 * N - 2,)
            d = np.abs(v - sol)
            assert d[:6 * N].max() <= TOL_TRAJ, (cfgname, i, d[:6 * N].max())
            assert d[6 * N:7 * N - 1].max() <= TOL_STEER, (cfgname, i, d[6 * N:7 * N - 1].max())
            assert d[7 * N - 1:].max() <= TOL_ACCEL, (cfgname, i, d[7 * N - 1:].max())


def test_restart_from_the_answer(pkg, warm_twin, golden_dir):
    opts = pkg.warm_opts_default(shift=0)
    for cfgname, params, b in golden_batches(pkg, golden_dir):
        cold = twin_warm_solve(warm_twin, params, b, opts)
        again = twin_warm_solve(warm_twin, params, b, opts, warm=cold["warm"], warm_status=cold["status"])
        print(cfgname, "iterations cold", cold["iters"].tolist(), "from the answer", again["iters"].tolist())
        assert np.array_equal(again["status"], cold["status"])
        assert np.abs(again["out"][6] - cold["out"][6]).max() <= TOL_STEER and np.abs(again["out"][7] - cold["out"][7]).max() <= TOL_ACCEL
        assert np.abs(again["out"][:6] - cold["out"][:6]).max() <= TOL_TRAJ
        assert (again["iters"] < cold["iters"]).all()


def test_fallbacks(pkg, warm_twin, golden_dir, host_twin):
    from helpers import twin_solve
    opts = pkg.warm_opts_default(shift=0)
    for cfgname, params, b in golden_batches(pkg, golden_dir):
        B = b["state"].shape[1]
        cold = twin_warm_solve(warm_twin, params, b, opts)
        # the cold solve of this build is the solve of the existing CPU build, bitwise
        plain = twin_solve(host_twin, params, b, want_traj=False)
        assert np.array_equal(plain["out"], cold["out"]) and np.array_equal(plain["status"], cold["status"]) and np.array_equal(plain["iters"], cold["iters"])
        # a warm_status entry != 0: bitwise the cold solve
        for bad in (1, 2, 4, 6):
            r = twin_warm_solve(warm_twin, params, b, opts, warm=cold["warm"], warm_status=np.full(B, bad, dtype=np.int32))
            assert np.array_equal(r["out"], cold["out"]) and np.array_equal(r["status"], cold["status"]) and np.array_equal(r["iters"], cold["iters"])
        # mixed validity: only the valid half is warm-started
        ws = np.zeros(B, dtype=np.int32); ws[::2] = 2
        r = twin_warm_solve(warm_twin, params, b, opts, warm=cold["warm"], warm_status=ws)
        assert np.array_equal(r["out"][:, ::2], cold["out"][:, ::2]) and np.array_equal(r["iters"][::2], cold["iters"][::2])
        assert (r["iters"][1::2] < cold["iters"][1::2]).all()
        # garbage: the cold solve's status, finite outputs within tolerance of cold, and no fewer iterations
        for name, g in zip(("nan", "far outside the bounds"), garbage_warm(params, cold["warm"])):
            r = twin_warm_solve(warm_twin, params, b, opts, warm=g)
            assert np.array_equal(r["status"], cold["status"]), name
            assert np.isfinite(r["out"]).all() and np.isfinite(r["warm"]).all(), name
            assert np.abs(r["out"][6] - cold["out"][6]).max() <= TOL_STEER and np.abs(r["out"][7] - cold["out"][7]).max() <= TOL_ACCEL, name
            assert np.abs(r["out"][:6] - cold["out"][:6]).max() <= TOL_TRAJ, name
            assert (r["iters"] >= cold["iters"]).all(), name
        # in place: warm_in is warm_out, warm_status is status
        w = cold["warm"].copy(); s = cold["status"].copy()
        sep = twin_warm_solve(warm_twin, params, b, opts, warm=cold["warm"], warm_status=cold["status"])
        inp = twin_warm_solve(warm_twin, params, b, opts, warm=w, warm_status=s, inplace=True)
        assert np.array_equal(inp["out"], sep["out"]) and np.array_equal(w, sep["warm"]) and np.array_equal(s, sep["status"])


def test_a_failed_warm_attempt_is_followed_by_the_cold_solve(pkg, warm_twin, golden_dir):
    """With max_iter = 3 a warm attempt from a three-iteration iterate mostly ends in MAXITER: the instance then gets the complete
    cold solve -- its status and outputs bitwise, the iterations of both attempts added."""
    opts = pkg.warm_opts_default(shift=0)
    for cfgname, params, b in golden_batches(pkg, golden_dir):
        p = params.copy(); p.max_iter = 3
        cold = twin_warm_solve(warm_twin, p, b, opts)
        assert (cold["status"] == 1).all() and (cold["iters"] == 3).all()
        r = twin_warm_solve(warm_twin, p, b, opts, warm=cold["warm"], warm_status=np.zeros(b["state"].shape[1], dtype=np.int32))
        done = r["status"] == 0                      # the warm attempt got there within the cap
        assert np.array_equal(r["status"][~done], cold["status"][~done])
        assert (r["iters"][~done] == 3 + cold["iters"][~done]).all()
        assert np.array_equal(r["out"][:, ~done], cold["out"][:, ~done])


def test_warm_abi(pkg):
    lib = pkg.library()
    assert lib.mpc_abi_version() == 5
    assert lib.mpc_warm_rows(10) == 9 * 22 and lib.mpc_warm_rows(25) == 24 * 22 and lib.mpc_warm_rows(2) < 0 and lib.mpc_warm_rows(65) < 0
    o = pkg.MpcWarmOpts()
    assert lib.mpc_warm_opts_default(C.byref(o)) == 0 and lib.mpc_warm_opts_default(None) == -1
    assert o.size == C.sizeof(pkg.MpcWarmOpts) and o.shift in (0, 1) and 0 < o.mu_init <= 0.1 and 0 < o.bound_push <= 1e-2 and o.duals in (0, 1) and o.reserved == 0
    from carnd_mpc_project_amd import _abi
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_amd.h"\nint main(){printf("%zu %zu %zu %zu %d %d\\n", sizeof(MpcWarmOpts), '
           'offsetof(MpcWarmOpts, mu_init), offsetof(MpcWarmOpts, duals), sizeof(MpcParams), MPC_WARM_REC, MPC_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(_abi.ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    assert out == [C.sizeof(pkg.MpcWarmOpts), pkg.MpcWarmOpts.mu_init.offset, pkg.MpcWarmOpts.duals.offset, C.sizeof(pkg.MpcParams), pkg.WARM_REC, 5]


def test_drop_in_warm_compiles(pkg):
    """tests/cpp/drop_in_warm_test.cpp builds against include/mpc_drop_in.hpp and the library (it runs in the GPU suite)."""
    from warm_helpers import build_drop_in_warm
    assert os.path.exists(build_drop_in_warm(pkg))
