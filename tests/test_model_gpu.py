"""Per-instance model values on the device (mpc_solve_batch_device_model, mpc_solve_batch_host_model, mpc_rollout_batch_device_model):
the MODEL builds of the lane kernel against the oracle solving every instance with its own OrcConfig, against the CPU build of the
same header (tests/host_twin, mpc_twin_solve) and against the plain entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ
from model_helpers import (INFEASIBLE, MODEL_FIELDS, assert_matches_oracle, draw_rows, load_model_twin, oracle_model_solve, population,
                           twin_model_solve)

pytestmark = pytest.mark.gpu

KEYS = ("out", "traj", "status", "iters")
F, I = -7777.25, -12345          # what the output arrays hold before a call


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model_twin():
    return load_model_twin()


@pytest.fixture(scope="module")
def fast(pkg, golden_dir):
    return pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))


@pytest.fixture(scope="module")
def pop(pkg, fast, waypoints):
    """the stated population (config-fast.json) with the oracle's and the CPU build's results, computed once"""
    b, model = population(pkg, fast, waypoints)
    return {"b": b, "model": model, "oracle": oracle_model_solve("config-fast.json", b, model)}


def _with(params, **kw):
    p = params.copy()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _abi_solve(pkg, mpc, b, model, dev, ld=None, traj=True, plain=False, weights=None):
    """One call through the C ABI with leading dimension `ld` (default B) and sentinels in every output array -> numpy, B columns
    (and "pad": whether the columns from B on still hold the sentinels).  plain: mpc_solve_batch_device instead."""
    import torch
    B = b["state"].shape[1]
    ld = ld or B
    N = mpc.N

    def wide(a):
        a = np.atleast_2d(np.asarray(a, dtype=np.float64))
        w = np.zeros((a.shape[0], ld)); w[:, :B] = a
        return torch.from_numpy(w).to(dev)
    st, cf, yl, yh = wide(b["state"]), wide(b["coeffs"]), wide(b["yaw_lo"]), wide(b["yaw_hi"])
    md = wide(model) if model is not None else None
    w = wide(weights) if weights is not None else None
    out = torch.full((9, ld), F, dtype=torch.float64, device=dev)
    tr = torch.full((2 * N, ld), F, dtype=torch.float64, device=dev) if traj else None
    status = torch.full((ld,), I, dtype=torch.int32, device=dev); iters = torch.full((ld,), I, dtype=torch.int32, device=dev)
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None
    if plain:
        rc = lib.mpc_solve_batch_device(mpc._h, B, ld, p(st), p(cf), p(yl), p(yh), p(w), p(out), p(tr), p(status), p(iters), stream)
    else:
        rc = lib.mpc_solve_batch_device_model(mpc._h, B, ld, p(st), p(cf), p(yl), p(yh), p(w), p(md), p(out), p(tr), p(status), p(iters), stream)
    assert rc == 0, (rc, lib.mpc_last_error())
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy() if t is not None else None
    o, t_, s, it = n(out), n(tr), n(status), n(iters)
    pad = bool((o[:, B:] == F).all() and (s[B:] == I).all() and (it[B:] == I).all() and (t_ is None or (t_[:, B:] == F).all()))
    return {"out": o[:, :B].copy(), "traj": t_[:, :B].copy() if traj else None, "status": s[:B].copy(), "iters": it[:B].copy(), "pad": pad}


def _assert_bitwise(a, c, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], c[k], equal_nan=True), (what, k)


def _assert_follows_twin(g, tw, what):
    """device against the CPU build of the same header (the reciprocals and the FMA contraction differ, so the bits do not carry
    over): the same status everywhere, and where the iteration counts agree the points agree within the tolerances"""
    assert np.array_equal(g["status"], tw["status"]), (what, np.where(g["status"] != tw["status"])[0][:8])
    both = (g["status"] == 0) & (g["iters"] == tw["iters"])
    print("%s vs CPU build: %d of %d with the same iteration count" % (what, int(both.sum()), both.size))
    assert both.any(), what
    assert np.abs(g["out"][6, both] - tw["out"][6, both]).max() <= TOL_STEER and np.abs(g["out"][7, both] - tw["out"][7, both]).max() <= TOL_ACCEL, what
    assert np.abs(g["out"][:6, both] - tw["out"][:6, both]).max() <= TOL_TRAJ and np.abs(g["traj"][:, both] - tw["traj"][:, both]).max() <= TOL_TRAJ, what


def _cols(b, idx):
    return {k: np.ascontiguousarray(v[..., idx]) for k, v in b.items()}


@pytest.mark.parametrize("B", [193, 7])
def test_parity_at_an_awkward_shape(pkg, fast, pop, model_twin, torch_dev, B):
    """B = 193 with ld = 256 (three full waves and one lane, a leading dimension that is not B) and B = 7: the device against the
    oracle -- its status on every instance, every instance it converges on within the tolerances -- and against the CPU build."""
    b, model = _cols(pop["b"], slice(0, B)), np.ascontiguousarray(pop["model"][:, :B])
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        g = _abi_solve(pkg, mpc, b, model, torch_dev, ld=256)
        st = mpc.stats()
    assert g["pad"]
    ref = {k: v[..., :B] for k, v in pop["oracle"].items()}
    assert_matches_oracle(g, ref, what="device B=%d ld=256" % B)
    _assert_follows_twin(g, twin_model_solve(model_twin, fast, b, model), "device B=%d" % B)
    # mpc_get_stats after a model call counts the INFEASIBLE instances
    assert st.batch == B and st.n_infeasible == int((ref["status"] == INFEASIBLE).sum()) and st.n_success == int((ref["status"] == 0).sum())
    assert st.n_pending == 0


def test_uniform_rows_against_the_plain_call(pkg, fast, pop, torch_dev):
    """Uniform rows equal to the handle's values, on a handle whose plain call is the single-phase fp64 lane kernel: the same status
    and iterations, outputs within the tolerances (and whether they are bitwise is printed: DESIGN.md 6k)."""
    p = _with(fast, wave_max_batch=-1, f64_f32_start=0)
    b = pop["b"]
    with pkg.BatchedMPC(p, 193, device=0) as mpc:
        plain = _abi_solve(pkg, mpc, b, None, torch_dev, plain=True)
        uni = _abi_solve(pkg, mpc, b, pkg.scenarios.model_rows(p, 193), torch_dev)
    assert np.array_equal(uni["status"], plain["status"]) and np.array_equal(uni["iters"], plain["iters"])
    ok = plain["status"] == 0
    assert ok.sum() >= 180
    assert np.abs(uni["out"][6, ok] - plain["out"][6, ok]).max() <= TOL_STEER and np.abs(uni["out"][7, ok] - plain["out"][7, ok]).max() <= TOL_ACCEL
    assert np.abs(uni["out"][:6, ok] - plain["out"][:6, ok]).max() <= TOL_TRAJ and np.abs(uni["traj"][:, ok] - plain["traj"][:, ok]).max() <= TOL_TRAJ
    print("uniform rows against the plain call, bitwise:", {k: bool(np.array_equal(uni[k], plain[k], equal_nan=True)) for k in KEYS})


def test_lane_compaction_moves_the_column_with_the_instance(pkg, fast, pop, torch_dev):
    """B = 8 256 (compaction runs from 8 192): the population tiled, a fresh draw of rows.  Bitwise the same call on a handle with
    lane_compact = 0, and every 16th instance against the oracle."""
    B = 8256
    idx = np.arange(B) % 193
    b = _cols(pop["b"], idx)
    model = draw_rows(fast, B, seed=6)
    got = []
    for lc in (fast.lane_compact, 0):
        with pkg.BatchedMPC(_with(fast, lane_compact=lc), B, device=0) as mpc:
            got.append(_abi_solve(pkg, mpc, b, model, torch_dev))
    _assert_bitwise(got[0], got[1], "lane compaction on / off")
    every = np.arange(0, B, 16)
    assert_matches_oracle(got[0], oracle_model_solve("config-fast.json", b, model, idx=every), idx=every, what="B=8256, every 16th")


def test_long_horizon_default_handle(pkg, golden_dir, waypoints, torch_dev):
    """config-stable.json with N = 25, dt = 0.05 and default parameters: the handle's ordinary solve starts in fp32.  A model call
    succeeds, is bitwise the same call on a handle with f64_f32_start = 0, and follows the oracle."""
    p = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"), N=25, dt=0.05)
    assert p.f64_f32_start == 2                      # (AUTO, in effect from N = 15)
    B = 1100
    b = pkg.scenarios.lake_track_batch(B, p, waypoints, seed=77)
    b = {k: np.ascontiguousarray(b[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    model = draw_rows(p, B, dts=(0.04, 0.05, 0.06))
    got = []
    for start in (p.f64_f32_start, 0):
        with pkg.BatchedMPC(_with(p, f64_f32_start=start), B, device=0) as mpc:
            got.append(_abi_solve(pkg, mpc, b, model, torch_dev))
    _assert_bitwise(got[0], got[1], "fp32-start handle / fp64 handle")
    some = np.arange(0, B, 17)[:64]
    assert_matches_oracle(got[0], oracle_model_solve("config-stable.json", b, model, idx=some, N=25), idx=some, what="N=25")


def test_second_order_correction(pkg, fast, golden_dir, torch_dev):
    """max_soc = 4 on the hard N = 10 instances, uniform rows: the MODEL+SOC build gives the status and iterations of the plain call
    on the same handle."""
    d = np.load(os.path.join(golden_dir, "soc_instances.npz"))
    b = {k: np.ascontiguousarray(d["n10_" + k]) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    B = b["state"].shape[1]
    p = _with(fast, max_soc=4, wave_max_batch=-1)
    with pkg.BatchedMPC(p, B, device=0) as mpc:
        plain = _abi_solve(pkg, mpc, b, None, torch_dev, plain=True)
        uni = _abi_solve(pkg, mpc, b, pkg.scenarios.model_rows(p, B), torch_dev)
    assert np.array_equal(uni["status"], plain["status"]) and np.array_equal(uni["iters"], plain["iters"])
    print("max_soc = 4, uniform rows against the plain call, bitwise:", {k: bool(np.array_equal(uni[k], plain[k], equal_nan=True)) for k in KEYS})


def test_rollout(pkg, fast, pop, torch_dev):
    """64 cars x 6 steps with per-car rows: hist, state, status and iters equal a loop of mpc_solve_batch_device_model fed as
    src/test.cpp feeds it, and every solve of 16 cars follows the oracle's own loop."""
    import torch
    B, steps = 64, 6
    # (cars the first solve accepts: a car that starts above its own speed limit has no closed loop)
    cars = np.where(pop["oracle"]["status"] == 0)[0][:B]
    b, model = _cols(pop["b"], cars), np.ascontiguousarray(pop["model"][:, cars])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dev)
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        state = t(b["state"])
        r = mpc.rollout_torch(state, t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), steps=steps, model=t(model))
        torch.cuda.synchronize()
        st = mpc.stats()
        hist, status, iters, final = r["hist"].cpu().numpy(), r["status"].cpu().numpy(), r["iters"].cpu().numpy(), state.cpu().numpy()
        cur = dict(b); lh = np.zeros((steps, 9, B)); ls = np.zeros(B, dtype=np.int32); li = np.zeros(B, dtype=np.int32)
        for k in range(steps):
            g = _abi_solve(pkg, mpc, cur, model, torch_dev, traj=False)
            lh[k] = g["out"]; ls = np.maximum(ls, g["status"]) if k else g["status"].copy(); li += g["iters"]
            cur = dict(cur, state=g["out"][:6].copy())
    assert np.array_equal(hist, lh) and np.array_equal(final, lh[-1, :6]) and np.array_equal(status, ls) and np.array_equal(iters, li)
    assert st.batch == B and st.n_success == int((status == 0).sum())
    for i in range(0, B, 4):
        over = {name: float(model[q, i]) for q, name in enumerate(MODEL_FIELDS)}
        cfg = O.load_config("config-fast.json", **over)
        cfg.yaw_low, cfg.yaw_high = float(b["yaw_lo"][i]), float(b["yaw_hi"][i])
        s = list(b["state"][:, i])
        for k in range(steps):
            stt, o9, _, _, _ = O.mpc_solve(cfg, s, b["coeffs"][:, i])
            assert stt == 0, (i, k, stt)
            assert abs(hist[k, 6, i] - o9[6]) <= TOL_STEER and abs(hist[k, 7, i] - o9[7]) <= TOL_ACCEL, (i, k)
            assert np.abs(hist[k, :6, i] - o9[:6]).max() <= TOL_TRAJ, (i, k)
            s = list(o9[:6])
    assert (status == 0).all()


def test_host_entry_point_and_python_arguments(pkg, fast, pop, torch_dev):
    """mpc_solve_batch_host_model (solve_numpy) and solve_torch(model=...) give the device call's results, bitwise."""
    import torch
    b, model = pop["b"], pop["model"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dev)
    with pkg.BatchedMPC(fast, 193, device=0) as mpc:
        ref = _abi_solve(pkg, mpc, b, model, torch_dev)
        host = mpc.solve_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], want_traj=True, model=model)
        r = mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), want_traj=True, model=t(model))
        torch.cuda.synchronize()
        dev = {k: r[k].cpu().numpy() for k in KEYS}
        with pytest.raises(ValueError):
            mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), model=t(model[:5]))
    _assert_bitwise(host, ref, "host entry point")
    _assert_bitwise(dev, ref, "solve_torch")


def test_refusals_and_forwarding(pkg, fast, pop, waypoints, torch_dev):
    import torch
    lib = pkg.library()
    # an fp32 handle is refused with a message, whatever else it is asked
    b1 = _cols(pop["b"], slice(0, 8))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch_dev)
    m = torch.from_numpy(pkg.scenarios.model_rows(fast, 8)).to(torch_dev)
    out = torch.zeros((9, 8), dtype=torch.float32, device=torch_dev); status = torch.zeros(8, dtype=torch.int32, device=torch_dev)
    with pkg.BatchedMPC(_with(fast, precision=pkg.PRECISION_F32), 8, device=0) as mpc:
        st, cf, yl, yh = f(b1["state"]), f(b1["coeffs"]), f(b1["yaw_lo"]), f(b1["yaw_hi"])
        for call in (lambda: lib.mpc_solve_batch_device_model(mpc._h, 8, 8, st.data_ptr(), cf.data_ptr(), yl.data_ptr(), yh.data_ptr(), None, m.data_ptr(),
                                                              out.data_ptr(), None, status.data_ptr(), None, None),
                     lambda: lib.mpc_rollout_batch_device_model(mpc._h, 8, 8, 2, st.data_ptr(), cf.data_ptr(), yl.data_ptr(), yh.data_ptr(), None,
                                                                m.data_ptr(), None, status.data_ptr(), None, None)):
            assert call() == -1
            assert b"fp64 handles only" in lib.mpc_last_error()
        torch.cuda.synchronize()
    # model = NULL is the plain entry point, bitwise: on the wave path (B = 192) and on the lane kernel (B = 1 061)
    for B in (192, 1061):
        sc = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=77)
        sc = {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
        with pkg.BatchedMPC(fast, B, device=0) as mpc:
            plain = _abi_solve(pkg, mpc, sc, None, torch_dev, plain=True)
            fwd = _abi_solve(pkg, mpc, sc, None, torch_dev)
        _assert_bitwise(fwd, plain, "model = NULL, B = %d" % B)
