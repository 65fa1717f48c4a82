"""IPOPT's second-order correction (MpcParams.max_soc) on the device: every kernel a max_soc > 0 solve can launch -- the lane kernel,
the one-instance-per-LPI-lanes kernel, the tail slices, the fp64 phase of both mixed-precision modes -- against each other (bitwise:
same header, same arithmetic) and against the CPU build of the header (tests/host_twin) and the oracle.  Instances: SURVEY's hard
ones from tests/golden/soc_instances.npz, padded with the survey population."""
import os

import numpy as np
import pytest

from helpers import TOL_ACCEL, TOL_STEER, twin_solve, twin_solve_mixed, twin_solve_mixed_f64

pytestmark = pytest.mark.gpu

KEYS = ("status", "iters", "out", "traj")
# Hard instances of the N = 10 survey population (position in the fixture) whose status differs between the solvers with
# max_soc = 4 and the oracle with max_soc = 4 (initial_state_rows = 1, the oracle's max_iter of 500 in both); tests/test_soc.py
# measures the same on the CPU build:
#    0 (population index 612): the oracle accepts one correction early and its line search later fails (113 iterations); the device
#      solver's own path converges (375 iterations, through the restart) -- without the correction the roles are reversed.
#   14 (7706, cte0 = 177 m): the oracle fails after 66 iterations with a correction that was never accepted; the device converges (61).
#   21 (9625, cte0 = 240 m) and 88 (34681, cte0 = -131 m): the device's line search fails with and without the correction, the
#      oracle converges with and without it: the two solvers' paths on these cars far off the fitted road part before the correction
#      acts (the same two fail at max_soc = 0).
STATUS_DIFFERS_FROM_ORACLE = {0, 14, 21, 88}


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def soc_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "soc_instances.npz"))


def _params(pkg, golden_dir, n25=False, **kw):
    p = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json" if n25 else "config-fast.json"), **(dict(N=25, dt=0.05) if n25 else {}))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _padded(pkg, d, params, waypoints, pop, B):
    """the fixture's instances of `pop` first, then survey instances up to B"""
    hard = {k: d["%s_%s" % (pop, k)] for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    n = hard["yaw_lo"].shape[0]
    pad = pkg.scenarios.lake_track_batch(B - n, params, waypoints, seed=91, stream=3, filtered="survey")
    return {k: np.ascontiguousarray(np.concatenate([hard[k], pad[k]], axis=-1)) for k in hard}, n


def _solve(pkg, params, b, dev, f32=False, mpc=None, outputs=None):
    import torch
    tdt = torch.float32 if f32 else torch.float64
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=tdt)
    B = b["state"].shape[1]
    own = mpc is None
    if own:
        mpc = pkg.BatchedMPC(params, B, device=0)
    r = mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), want_traj=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in r.items()}
    if own:
        mpc.close()
    return out


def _assert_bitwise(a, c, what):
    for k in KEYS:
        assert np.array_equal(a[k], c[k], equal_nan=True), (what, k, np.where(a["status"] != c["status"])[0][:5])


def _assert_follows_twin(g, tw, n_hard, what):
    """device against the CPU build of the same header: the reciprocals (v_rcp + Newton steps on the device, IEEE division on the
    CPU) and the FMA contraction differ, so the bits do not carry over -- the statuses, and the points where both take the same
    number of iterations, do"""
    same_status = g["status"] == tw["status"]
    assert same_status.mean() >= 0.99, (what, int((~same_status).sum()))
    assert (g["status"][:n_hard] == 0).sum() >= (tw["status"][:n_hard] == 0).sum() - 2, what
    both = (g["status"] == 0) & (tw["status"] == 0) & (g["iters"] == tw["iters"])
    assert both.mean() >= 0.9, (what, float(both.mean()))
    assert np.max(np.abs(g["out"][6, both] - tw["out"][6, both])) <= TOL_STEER, what
    assert np.max(np.abs(g["out"][7, both] - tw["out"][7, both])) <= TOL_ACCEL, what


def test_lane_kernel_with_the_correction(pkg, host_twin, golden_dir, waypoints, soc_fixture, torch_dev):
    """The lane-per-instance kernel (wave_max_batch = -1) with max_soc = 4: it corrects (fewer iterations on the hard instances than
    with max_soc = 0, more of them converged, the rest of the batch untouched) and follows the CPU build of the header."""
    p4 = _params(pkg, golden_dir, max_soc=4, wave_max_batch=-1)
    b, n = _padded(pkg, soc_fixture, p4, waypoints, "n10", 4096)
    g4 = _solve(pkg, p4, b, torch_dev)
    g0 = _solve(pkg, _params(pkg, golden_dir, wave_max_batch=-1), b, torch_dev)
    assert g4["iters"][:n].sum() < g0["iters"][:n].sum()
    assert (g4["status"][:n] == 0).sum() > (g0["status"][:n] == 0).sum()
    changed = (g4["iters"] != g0["iters"]) | np.any(g4["out"] != g0["out"], axis=0)
    assert changed[:n].sum() >= n // 2 and changed[n:].mean() < 0.05
    _assert_follows_twin(g4, twin_solve(host_twin, p4, b), n, "lane")


@pytest.mark.parametrize("pop,lpi", [("n10", 16), ("n10", 32), ("n10", 64), ("n25", 32), ("n25", 64)])
def test_wave_kernel_with_the_correction_is_bitwise_the_lane_kernel(pkg, golden_dir, waypoints, soc_fixture, torch_dev, pop, lpi, monkeypatch):
    """mpc_solve_wave_kernel's SOC build at 16 / 32 / 64 lanes per instance (the SOC records in LDS behind the stage records, lane k
    preparing stage k's corrected residual): bitwise the lane kernel's results."""
    n25 = pop == "n25"
    b = {k: soc_fixture["%s_%s" % (pop, k)] for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    lane = _solve(pkg, _params(pkg, golden_dir, n25, max_soc=4, wave_max_batch=-1, f64_f32_start=0), b, torch_dev)
    monkeypatch.setenv("MPC_WAVE_LPI", str(lpi))
    wave = _solve(pkg, _params(pkg, golden_dir, n25, max_soc=4, wave_max_batch=4096, f64_f32_start=0), b, torch_dev)
    _assert_bitwise(lane, wave, (pop, lpi))
    if not n25:
        assert (lane["status"] == 0).sum() >= len(lane["status"]) - 8


def test_deferred_tails_with_the_correction_are_bitwise_the_single_launch(pkg, golden_dir, waypoints, soc_fixture, torch_dev):
    """tail_cut = MPC_TAIL_AUTO with three batches in flight, each made final through mpc_tail_poll: the stragglers -- the hard
    instances, where the corrections happen -- finish in the SOC build of the tail slices, bitwise what one launch writes."""
    import time
    import torch
    p = _params(pkg, golden_dir, max_soc=4)
    b, n = _padded(pkg, soc_fixture, p, waypoints, "n10", 8192)
    ref = _solve(pkg, p, b, torch_dev)
    q = p.copy(); q.tail_cut = -1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_dev, dtype=torch.float64)
    ins = [t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"])]
    B = b["state"].shape[1]
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        outs = [mpc.alloc_outputs(B, torch_dev, True) for _ in range(3)]
        ids = []
        for k in range(3):
            mpc.solve_torch(*ins, outputs=outs[k])
            ids.append(mpc.last_batch_id())
        deadline = time.time() + 120
        for i in ids:
            while not mpc.tail_poll(i):
                assert time.time() < deadline, "batch %d not final" % i
                time.sleep(0.001)
        torch.cuda.synchronize()
        for k in range(3):
            got = {kk: v.cpu().numpy() for kk, v in outs[k].items()}
            _assert_bitwise(ref, got, ("tail", k))
    assert (ref["iters"][:n] > 20).sum() > n // 2          # (the stragglers the cut hands over include the corrected instances)


def test_mixed_precision_f64_phase_corrects(pkg, host_twin, golden_dir, waypoints, soc_fixture, torch_dev):
    """N = 25 with f64_f32_start AUTO (the two-launch solve: fp32 start, fp64 finish): the fp64 phase honours max_soc -- its SOC build
    follows the CPU replay of the same two phases; and on an F32 handle with f32_finish = 1 the fp64 finish does the same."""
    p = _params(pkg, golden_dir, True, max_soc=4, wave_max_batch=-1)
    assert p.f64_f32_start == 2
    b, n = _padded(pkg, soc_fixture, p, waypoints, "n25", 2048)
    g4 = _solve(pkg, p, b, torch_dev)
    g0 = _solve(pkg, _params(pkg, golden_dir, True, wave_max_batch=-1), b, torch_dev)
    assert g4["iters"][:n].sum() < g0["iters"][:n].sum()
    _assert_follows_twin(g4, twin_solve_mixed_f64(host_twin, p, b), n, "f64_f32_start")
    q = _params(pkg, golden_dir, max_soc=4, wave_max_batch=-1)
    q.precision = pkg.PRECISION_F32; q.f32_finish = 1
    bb, m = _padded(pkg, soc_fixture, q, waypoints, "n10", 2048)
    f4 = _solve(pkg, q, bb, torch_dev, f32=True)
    q0 = q.copy(); q0.max_soc = 0
    f0 = _solve(pkg, q0, bb, torch_dev, f32=True)
    assert not np.array_equal(f4["iters"][:m], f0["iters"][:m])
    tw = twin_solve_mixed(host_twin, q, bb)
    _assert_follows_twin(f4, tw, m, "f32_finish")


def test_live_handle_switched_back_to_off(pkg, golden_dir, waypoints, soc_fixture, torch_dev):
    """mpc_set_params on a live handle: 0 -> 4 allocates the SOC records and corrects; 4 -> 0 returns exactly today's results."""
    p = _params(pkg, golden_dir, wave_max_batch=-1)
    b, n = _padded(pkg, soc_fixture, p, waypoints, "n10", 2048)
    with pkg.BatchedMPC(p, 2048, device=0) as mpc:
        r0 = _solve(pkg, p, b, torch_dev, mpc=mpc)
        q = p.copy(); q.max_soc = 4
        mpc.set_params(q)
        r4 = _solve(pkg, q, b, torch_dev, mpc=mpc)
        mpc.set_params(p)
        r0b = _solve(pkg, p, b, torch_dev, mpc=mpc)
    fresh4 = _solve(pkg, q, b, torch_dev)
    _assert_bitwise(r0, r0b, "4 -> 0")
    _assert_bitwise(r4, fresh4, "0 -> 4")
    assert not np.array_equal(r0["iters"], r4["iters"])


def test_survey_batch_statuses_match_the_oracle(pkg, golden_dir, waypoints, soc_fixture, torch_dev):
    """One 65 536-instance survey batch (the default launch, max_soc = 4, initial_state_rows = 1, the oracle's max_iter): on the hard
    instances of the fixture the statuses are the oracle's with max_soc = 4, except STATUS_DIFFERS_FROM_ORACLE."""
    p = _params(pkg, golden_dir, max_soc=4, initial_state_rows=1, max_iter=500)
    b = pkg.scenarios.lake_track_batch(65536, p, waypoints, stream=3, filtered="survey")
    idx = soc_fixture["n10_index"]
    assert np.array_equal(b["state"][:, idx], soc_fixture["n10_state"])
    g = _solve(pkg, p, b, torch_dev)
    st = g["status"][idx]
    differs = set(np.where(st != soc_fixture["n10_oracle_status4"])[0].tolist())
    assert differs <= STATUS_DIFFERS_FROM_ORACLE, sorted(differs - STATUS_DIFFERS_FROM_ORACLE)
    assert (st == 0).sum() >= (soc_fixture["n10_oracle_status4"] == 0).sum() - 2
    assert (g["status"] == 0).mean() > 0.99
