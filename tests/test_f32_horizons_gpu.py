"""The fp32 record (Layout<float>) on the device at horizons other than N = 10: the three ways a solve iterates on it --
  1. MPC_PRECISION_F32 handles with f32_finish = 1 (the two-launch lane path at every launch size),
  2. fp64 handles whose solve starts in fp32 (f64_f32_start = AUTO, the default, from N = 15; wave_max_batch = -1 here so that a
     launch of 165 reaches the two-launch solve),
  3. the pure fp32 wave kernel (f32_finish = 0, launches of at most 1 024) with 16, 32 and 64 lanes per instance,
and 4. what the default AUTO means for a caller: at N >= 15 the bits of a result depend on the launch size (wave kernel, all fp64,
up to wave_max_batch; fp32 start above) within the fp64 tolerances, and MPC_F32_START_OFF makes them identical.

One population per horizon: lake_track_batch(165, ..., seed = 60 + N) -- two full wavefronts and one of 37 lanes.  The CPU twin
(tests/host_twin) converges on all 165 of every row in all three of its forms; it has no staging, no counted waits, no workspace tiles
and no lane groups, which is what these tests add.  Every tolerance is one the project states (helpers.TOL_*, F32_TOL_*, the
best-effort bounds of test_f32.test_f32_pure_long_horizons_are_best_effort); none comes from what is measured here.  Each case prints
its measured maxima before it asserts; `python tests/test_f32_horizons_gpu.py [file]` runs every case and writes them as JSON
(profiles/f32_horizons.json)."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from helpers import (F32_TOL_ACCEL, F32_TOL_STATE, F32_TOL_STEER, F32_TOL_TRAJ, TOL_ACCEL, TOL_STEER, TOL_TRAJ, assert_parity, f32_forks,
                     oracle_solve_batch, twin_solve_mixed, twin_solve_mixed_f64)
from test_f32 import ZERO_V, _check_f32

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
B = 165                                   # 64 + 64 + 37
ROWS = {3: ("config-fast.json", 0.1), 4: ("config-fast.json", 0.05), 14: ("config-fast.json", 0.1), 15: ("config-fast.json", 0.1),
        17: ("config-stable.json", 0.07), 18: ("config-stable.json", 0.07), 25: ("config-stable.json", 0.05),
        34: ("config-stable.json", 0.04), 40: ("config-fast.json", 0.025), 64: ("config-stable.json", 0.02)}
KEYS = ("state", "coeffs", "yaw_lo", "yaw_hi")
BITS = ("status", "iters", "out", "traj")
PURE_BEST_EFFORT_STEER, PURE_BEST_EFFORT_STATE = 2e-3, 2e-2       # test_f32_pure_long_horizons_are_best_effort
MEASURED = {}


def _params(pkg, N, **over):
    config, dt = ROWS[N]
    p = pkg.params_from_json(os.path.join(GOLDEN, config), N=N, dt=dt)
    for k, v in over.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _population(pkg, N, sweep):
    """The 165 instances of horizon N (and the weight sweep with velocity weight 0 of the N = 25 sweep case)."""
    params = _params(pkg, N)
    wp = pkg.scenarios.load_waypoints(os.path.join(GOLDEN, "lake_track_waypoints.csv"))
    b = pkg.scenarios.lake_track_batch(B, params, wp, seed=60 + N)
    w = pkg.scenarios.weight_sweep(B, params, seed=60 + N, velocity_weights=ZERO_V) if sweep else None
    return b, w


def _sample(N):
    """The instances that go to the dense oracle: 12 up to N = 40, 4 at N = 64 -- the first, the last (lane 36 of the partly filled
    wavefront) and evenly between."""
    return [int(i) for i in np.linspace(0, B - 1, 4 if N > 40 else 12).round()]


@functools.lru_cache(maxsize=None)
def _oracle(pkg, N, sweep):
    """The oracle's answers on _sample(N): computed once, shared by the cases of this horizon, never written to."""
    config, dt = ROWS[N]
    b, w = _population(pkg, N, sweep)
    return oracle_solve_batch(O.load_config(config, N=N, dt=dt), b, _sample(N), weights=w)


def _cols(r, idx):
    return {k: (v[..., idx] if v is not None else None) for k, v in r.items()}


def _solve(mpc, b, w=None, n=None):
    """One device call on `mpc` (the first n instances; trajectories on), as numpy arrays."""
    import torch
    dt = torch.float32 if mpc.f32 else torch.float64
    n = b["state"].shape[1] if n is None else n
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[..., :n])).to("cuda:0", dtype=dt)
    r = mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), weights=t(w) if w is not None else None, want_traj=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _solve_once(pkg, params, b, w=None, n=None):
    with pkg.BatchedMPC(params, B if n is None else n, device=0) as mpc:
        return _solve(mpc, b, w, n)


def _maxima(got, ref):
    """Largest differences over the instances both sides converged on; the statuses that differ and each side's failures."""
    ok = (got["status"] == 0) & (ref["status"] == 0)
    g, r = got["out"].astype(np.float64)[:, ok], ref["out"].astype(np.float64)[:, ok]
    m = lambda x: float(x.max()) if x.size else 0.0
    return {"steer": m(np.abs(g[6] - r[6])), "accel": m(np.abs(g[7] - r[7])), "state": m(np.abs(g[:6] - r[:6])),
            "traj": m(np.abs(got["traj"].astype(np.float64) - ref["traj"].astype(np.float64))[:, ok]), "compared": int(ok.sum()),
            "status_differs": int((got["status"] != ref["status"]).sum()), "failures": int((got["status"] != 0).sum()),
            "ref_failures": int((ref["status"] != 0).sum())}


def _rounded(x):
    return {k: _rounded(v) for k, v in x.items()} if isinstance(x, dict) else float("%.3g" % x) if isinstance(x, float) else x


def _record(case, **figures):
    figures = _rounded(figures)
    MEASURED[case] = figures
    print("%s: %s" % (case, json.dumps(figures)))


def _same_bits(a, b, what):
    for k in BITS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, np.where(a["status"] != b["status"])[0][:8])


# ---- 1. MPC_PRECISION_F32, f32_finish = 1 ------------------------------------------------------------------------------------------
def run_mixed(pkg, twin, N, sweep=False):
    case = "f32_finish N=%d%s" % (N, " weight sweep" if sweep else "")
    params = _params(pkg, N, precision=pkg.PRECISION_F32, f32_finish=1)
    p64 = _params(pkg, N)
    b, w = _population(pkg, N, sweep)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        r32 = _solve(mpc, b, w)
        again = _solve(mpc, b, w)
        host = (mpc.solve_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], weights=w, want_traj=True) if N in (25, 64) and not sweep
                else None)
    r64 = _solve_once(pkg, p64, b, w)
    tw = twin_solve_mixed(twin, params, b, weights=w)
    idx, ref = _sample(N), _oracle(pkg, N, sweep)
    fork, wrong = f32_forks(r32, r64, (r32["status"] == 0) & (r64["status"] == 0))
    _record(case, device_fp64=_maxima(r32, r64), twin=_maxima(r32, tw), oracle=_maxima(_cols(r32, idx), ref), forks=int(fork.sum()),
            wrong=int(wrong.sum()), iters_mean=float("%.4g" % r32["iters"].mean()), twin_iters_mean=float("%.4g" % tw["iters"].mean()))
    assert r32["out"].dtype == np.float32 and r32["traj"].dtype == np.float32
    _check_f32(r32, r64, case + ", HIP mixed vs HIP fp64", B)
    assert np.array_equal(r32["status"], tw["status"]), (case, np.where(r32["status"] != tw["status"])[0][:8])
    _check_f32(_cols(r32, idx), ref, case + ", HIP mixed vs oracle", len(idx))
    _same_bits(again, r32, case + ", second call on the handle")
    if host is not None:
        _same_bits(host, r32, case + ", mpc_solve_batch_host_f32")


@pytest.mark.parametrize("N", [3, 4, 17, 18, 25, 34, 40, 64])
def test_f32_finish_at_horizon(pkg, host_twin, N):
    """mpc_solve_batch_device_f32, f32_finish = 1, on all 165 instances: status and F32_TOL_* against the fp64 device path (forks bounded
    as in _check_f32), the twin's status on every instance, F32_TOL_* against the oracle on the sample, a second call on the handle
    bit for bit, and at N = 25 and 64 the host form bit for bit."""
    run_mixed(pkg, host_twin, N)


def test_f32_finish_weight_sweep_with_zero_velocity_weight_at_N25(pkg, host_twin):
    """The same at N = 25 with per-instance weights, velocity weight 0 included."""
    run_mixed(pkg, host_twin, 25, sweep=True)


# ---- 2. the fp32 start of an fp64 handle -------------------------------------------------------------------------------------------
def run_start(pkg, twin, N, rows=0):
    case = "f32 start N=%d%s" % (N, " initial_state_rows" if rows else "")
    auto = _params(pkg, N, wave_max_batch=-1, initial_state_rows=rows)
    assert auto.f64_f32_start == 2 and pkg.PRECISION_F64 == auto.precision          # MPC_F32_START_AUTO, as shipped
    off = auto.copy(); off.f64_f32_start = 0
    b, _ = _population(pkg, N, False)
    r, r0 = _solve_once(pkg, auto, b), _solve_once(pkg, off, b)
    if N < 15:                      # the lower side of MPC_F32_START_AUTO_N: the single-phase solve
        _record(case, bitwise_single_phase=bool(all(np.array_equal(r[k], r0[k], equal_nan=True) for k in BITS)))
        _same_bits(r, r0, case + ", AUTO below N = 15")
        return
    tw = twin_solve_mixed_f64(twin, auto, b)
    idx, ref = _sample(N), _oracle(pkg, N, False)
    _record(case, single_phase=_maxima(r, r0), twin=_maxima(r, tw), oracle=_maxima(_cols(r, idx), ref),
            oracle_single_phase=_maxima(_cols(r0, idx), ref), out_bitwise_single_phase=bool(np.array_equal(r["out"], r0["out"])),
            iters_mean=float("%.4g" % r["iters"].mean()), single_phase_iters_mean=float("%.4g" % r0["iters"].mean()))
    assert (tw["status"] == 0).all(), (case, "the reference:", np.bincount(tw["status"]))
    assert np.array_equal(r["status"], r0["status"]), (case, np.where(r["status"] != r0["status"])[0][:8])
    assert np.array_equal(r["status"], tw["status"]), (case, np.where(r["status"] != tw["status"])[0][:8])
    assert_parity(r["out"], r0["out"], r["traj"], r0["traj"], case + ", fp32 start vs single phase")
    assert (ref["status"] == 0).all()
    assert_parity(r["out"][:, idx], ref["out"], r["traj"][:, idx], ref["traj"], case + ", fp32 start vs oracle")
    assert not np.array_equal(r["out"], r0["out"]), case + ": bitwise the single-phase solve -- the fp32 phase did not run"


@pytest.mark.parametrize("N", [14, 15, 18, 34, 40, 64])
def test_f32_start_at_horizon(pkg, host_twin, N):
    """An fp64 handle with default f64_f32_start and wave_max_batch = -1.  N = 14: bitwise f64_f32_start = 0.  N >= 15: the status of the
    single-phase device solve and of the twin's two phases, TOL_* against the single-phase solve on all 165 and against the oracle
    on the sample, and an `out` that is not the single-phase solve's bit for bit (the fp32 phase ran: the twin differs on every row)."""
    run_start(pkg, host_twin, N)


def test_f32_start_with_initial_state_rows_at_N25(pkg, host_twin):
    """N = 25 with initial_state_rows = 1: the rows' multipliers cross from the fp32 to the fp64 solver."""
    run_start(pkg, host_twin, 25, rows=1)


# ---- 3. the pure fp32 wave kernel at every group size ------------------------------------------------------------------------------
def run_pure_wave(pkg, N):
    case = "f32 pure wave N=%d" % N
    wave = _params(pkg, N, precision=pkg.PRECISION_F32, f32_finish=0)
    assert wave.wave_max_batch == 0                                                  # the default limit: 1 024
    lane = wave.copy(); lane.wave_max_batch = -1
    b, _ = _population(pkg, N, False)
    rw, rl = _solve_once(pkg, wave, b), _solve_once(pkg, lane, b)
    r8 = _solve_once(pkg, wave, b, n=8)                                              # a whole wavefront per instance
    r64 = _solve_once(pkg, _params(pkg, N), b)
    d = _maxima(rw, r64)
    _record(case, lanes_per_instance=16 if N <= 17 else 32 if N <= 33 else 64, device_fp64=d, statuses=np.bincount(rw["status"], minlength=5).tolist(),
            bitwise_lane_kernel=bool(all(np.array_equal(rw[k], rl[k], equal_nan=True) for k in BITS)),
            bitwise_whole_wave=bool(all(np.array_equal(r8[k], rw[k][..., :8], equal_nan=True) for k in BITS)))
    _same_bits(rw, rl, case + ", wave kernel vs lane kernel")
    assert set(np.unique(rw["status"])) <= {0, 1, 2}, np.bincount(rw["status"])
    assert (rw["status"] != 0).sum() <= 2, np.bincount(rw["status"])
    assert d["steer"] <= PURE_BEST_EFFORT_STEER and d["state"] <= PURE_BEST_EFFORT_STATE, d
    _same_bits(r8, _cols(rw, slice(0, 8)), case + ", B = 8")


@pytest.mark.parametrize("N", [3, 18, 34])
def test_f32_pure_wave_kernel_at_every_group_size(pkg, N):
    """f32_finish = 0 on a default handle, B = 165: mpc_solve_wave_kernel<float, LPI> with 16, 32 and 64 lanes per instance, the last
    wavefront partly filled.  Bitwise the lane kernel (wave_max_batch = -1) in status, iters, out and traj; statuses within {0, 1, 2},
    at most 2 of 165 not solved (a cap: the twin has at most 1); where it and fp64 converge, within the best-effort bounds of the pure
    mode at long horizons; and B = 8 is bitwise the first 8 columns."""
    run_pure_wave(pkg, N)


# ---- 4. the default's dependence on the launch size --------------------------------------------------------------------------------
LAUNCH_SEED = 85          # (twin_solve converges on all 1 125 instances of this seed)


def run_launch_size(pkg):
    case = "launch size N=25"
    params = _params(pkg, 25)
    assert params.f64_f32_start == 2 and params.wave_max_batch == 0
    wp = pkg.scenarios.load_waypoints(os.path.join(GOLDEN, "lake_track_waypoints.csv"))
    big = pkg.scenarios.lake_track_batch(1125, params, wp, seed=LAUNCH_SEED)
    res = {}
    for start in (2, 0):
        q = params.copy(); q.f64_f32_start = start
        with pkg.BatchedMPC(q, 1125, device=0) as mpc:
            alone = _solve(mpc, big, n=64)                    # a launch of 64: the wave kernel, every iteration in fp64
            inside = _cols(_solve(mpc, big), slice(0, 64))    # a launch of 1 125 = 1 024 + 64 + 37: the two-launch solve (fp32 start)
        res[start] = (alone, inside)
    idx = [int(i) for i in np.linspace(0, 63, 8).round()]
    ref = oracle_solve_batch(O.load_config("config-stable.json", N=25, dt=0.05), big, idx)
    (alone, inside), (alone0, inside0) = res[2], res[0]
    _record(case, alone_vs_inside=_maxima(alone, inside), alone_vs_oracle=_maxima(_cols(alone, idx), ref), inside_vs_oracle=_maxima(_cols(inside, idx), ref),
            default_bitwise=bool(np.array_equal(alone["out"], inside["out"])),
            start_off_bitwise=bool(all(np.array_equal(alone0[k], inside0[k], equal_nan=True) for k in BITS)))
    assert np.array_equal(alone["status"], inside["status"]) and (ref["status"] == 0).all()
    assert_parity(alone["out"], inside["out"], alone["traj"], inside["traj"], case + ", launch of 64 vs inside a launch of 1 125")
    assert_parity(alone["out"][:, idx], ref["out"], alone["traj"][:, idx], ref["traj"], case + ", launch of 64 vs oracle")
    assert_parity(inside["out"][:, idx], ref["out"], inside["traj"][:, idx], ref["traj"], case + ", inside a launch of 1 125 vs oracle")
    _same_bits(alone0, inside0, case + ", MPC_F32_START_OFF")
    _same_bits(alone0, alone, case + ", the wave kernel does not read f64_f32_start")


def test_default_results_depend_on_the_launch_size_within_tolerance_and_not_with_f32_start_off(pkg):
    """A default handle at N = 25: instances 0 .. 63 solved alone (wave kernel, all fp64) and inside a launch of 1 125 (fp32 start) have
    equal statuses and agree within TOL_*, each follows the oracle; with MPC_F32_START_OFF the two are bitwise equal (include/mpc_amd.h
    and INTEGRATION.md say so to callers)."""
    run_launch_size(pkg)


def run_all(pkg, twin):
    """Every case, in the order of the tests; a failing one is recorded and does not stop the rest."""
    calls = ([(run_mixed, (pkg, twin, N)) for N in (3, 4, 17, 18, 25, 34, 40, 64)] + [(run_mixed, (pkg, twin, 25, True))] +
             [(run_start, (pkg, twin, N)) for N in (14, 15, 18, 34, 40, 64)] + [(run_start, (pkg, twin, 25, 1))] +
             [(run_pure_wave, (pkg, N)) for N in (3, 18, 34)] + [(run_launch_size, (pkg,))])
    failed = {}
    for fn, args in calls:
        try:
            fn(*args)
        except AssertionError as e:
            failed["%s%r" % (fn.__name__, tuple(a for a in args if a is not pkg and a is not twin))] = str(e)[:400]
    return {"what": "measured maxima of tests/test_f32_horizons_gpu.py on an MI355X (gfx950): 165 lake-track instances per horizon (seed 60 + N), "
                    "the device against the fp64 device path, the CPU twin and the oracle sample, over the instances both sides converge on",
            "how": "python tests/test_f32_horizons_gpu.py profiles/f32_horizons.json",
            "asserted": {"F32_TOL_STEER": F32_TOL_STEER, "F32_TOL_ACCEL": F32_TOL_ACCEL, "F32_TOL_STATE": F32_TOL_STATE, "F32_TOL_TRAJ": F32_TOL_TRAJ,
                         "TOL_STEER": TOL_STEER, "TOL_ACCEL": TOL_ACCEL, "TOL_TRAJ": TOL_TRAJ, "pure best effort steer": PURE_BEST_EFFORT_STEER,
                         "pure best effort state": PURE_BEST_EFFORT_STATE, "pure failures of 165": 2},
            "cases": dict(MEASURED), "failed": failed}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import __graft_entry__ as G
    from helpers import load_twin
    doc = json.dumps(run_all(G.load_package(), load_twin()), indent=1)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(doc + "\n")
    else:
        print(doc)
