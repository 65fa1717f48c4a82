"""Warm starts and closed loops with per-instance model values on the device (mpc_solve_batch_device_warm_model, _host_warm_model,
mpc_rollout_batch_device_warm_model, mpc_rollout_batch_device_fused_model): the WARM+MODEL and ROLL+MODEL builds of the lane kernel
against the cold model entry points, the oracle solving every instance with its own OrcConfig, the CPU build of the same header
(tests/host_twin, mpc_twin_solve / mpc_twin_rollout) and the stepwise loops the fused call stands for.  Every output array holds sentinels before a call."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ
from model_helpers import INFEASIBLE, assert_matches_oracle, draw_rows, oracle_model_solve, population
from model_loop_helpers import (MODES, WARM_REC, assert_loops_follow_oracle, load_model_loop_twin, oracle_model_loops, steering_outside,
                                twin_warm_model_solve)
from warm_helpers import garbage_warm

pytestmark = pytest.mark.gpu

KEYS = ("out", "traj", "status", "iters")
F, I = -7777.25, -12345          # what the output arrays hold before a call
STAT_FIELDS = ("batch", "n_success", "n_maxiter", "n_linesearch", "n_infeasible", "n_numeric", "n_acceptable", "iter_sum", "iter_max", "n_pending")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return load_model_loop_twin()


@pytest.fixture(scope="module")
def fast(pkg, golden_dir):
    return pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))


@pytest.fixture(scope="module")
def pop(pkg, fast, waypoints):
    """the stated population (config-fast.json) with the oracle's cold results, computed once"""
    b, model = population(pkg, fast, waypoints)
    return {"b": b, "model": model, "oracle": oracle_model_solve("config-fast.json", b, model)}


def _with(params, **kw):
    p = params.copy()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _cols(b, idx):
    return {k: np.ascontiguousarray(v[..., idx]) for k, v in b.items()}


def _wide(a, ld, dev, dtype=np.float64):
    import torch
    a = np.atleast_2d(np.asarray(a, dtype=dtype))
    w = np.zeros((a.shape[0], ld), dtype=dtype); w[:, :a.shape[1]] = a
    return torch.from_numpy(w).to(dev)


def _solve(pkg, mpc, b, model, dev, kind="warm_model", ld=None, warm=None, warm_status=None, inplace=None, opts=None, weights=None, expect=0):
    """One solve through the C ABI with leading dimension ld (default B) and sentinels in every output array -> numpy, B columns,
    "pad" (whether the columns from B on still hold the sentinels -- the warm buffer's too) and "dev" (the warm and status tensors,
    to hand to a later call as `inplace`: then they are warm_in = warm_out and warm_status = status of that call).
    kind: "warm_model", "warm" (mpc_solve_batch_device_warm; model must be None) or "model" (mpc_solve_batch_device_model)."""
    import torch
    B = b["state"].shape[1]
    ld = ld or B
    N, rows = mpc.N, mpc.warm_rows()
    st, cf, yl, yh = (_wide(b[k], ld, dev) for k in ("state", "coeffs", "yaw_lo", "yaw_hi"))
    md = _wide(model, ld, dev) if model is not None else None
    w = _wide(weights, ld, dev) if weights is not None else None
    out = torch.full((9, ld), F, dtype=torch.float64, device=dev)
    tr = torch.full((2 * N, ld), F, dtype=torch.float64, device=dev)
    iters = torch.full((ld,), I, dtype=torch.int32, device=dev)
    if inplace is not None:
        w_in = w_out = inplace["warm"]; w_st = status = inplace["status"]
    else:
        w_in = _wide(warm, ld, dev) if warm is not None else None
        w_st = _wide(warm_status, ld, dev, np.int32)[0] if warm_status is not None else None
        w_out = torch.full((rows, ld), F, dtype=torch.float64, device=dev)
        status = torch.full((ld,), I, dtype=torch.int32, device=dev)
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None
    o = C.byref(opts) if opts is not None else None
    head = (mpc._h, B, ld, p(st), p(cf), p(yl), p(yh), p(w))
    tail = (p(out), p(tr), p(status), p(iters), stream)
    if kind == "model":
        rc = lib.mpc_solve_batch_device_model(*head, p(md), *tail)
    elif kind == "warm":
        assert model is None
        rc = lib.mpc_solve_batch_device_warm(*head, p(w_in), p(w_st), p(w_out), ld, o, *tail)
    else:
        rc = lib.mpc_solve_batch_device_warm_model(*head, p(md), p(w_in), p(w_st), p(w_out), ld, o, *tail)
    assert rc == expect, (rc, lib.mpc_last_error())
    torch.cuda.synchronize()
    if expect:
        return None
    o_, t_, s_, it_, wm = (x.cpu().numpy() for x in (out, tr, status, iters, w_out))
    pad = bool((o_[:, B:] == F).all() and (t_[:, B:] == F).all() and (it_[B:] == I).all())
    if inplace is None:
        pad = pad and bool((s_[B:] == I).all()) and (kind == "model" or bool((wm[:, B:] == F).all()))
    return {"out": o_[:, :B].copy(), "traj": t_[:, :B].copy(), "status": s_[:B].copy(), "iters": it_[:B].copy(), "warm": wm[:, :B].copy(),
            "pad": pad, "dev": {"warm": w_out, "status": status}}


def _roll(pkg, mpc, sc, model, steps, dev, kind, warm_start=False, opts=None, weights=None, want_hist=True, ld=None, expect=0):
    """One rollout through the C ABI: kind "fused" (mpc_rollout_batch_device_fused_model), "stepwise" (mpc_rollout_batch_device_model or
    _warm_model) or "plain_fused" / "plain" (the entry points without _model; model must be None, passed to the _model entry point when
    `kind` ends in "_null").  Returns hist, state, status, iters as numpy, all ld columns."""
    import torch
    B = sc["state"].shape[1]
    ld = ld or B
    state, coeffs, ylo, yhi = (_wide(sc[k], ld, dev) for k in ("state", "coeffs", "yaw_lo", "yaw_hi"))
    md = _wide(model, ld, dev) if model is not None else None
    w = _wide(weights, ld, dev) if weights is not None else None
    hist = torch.full((steps, 9, ld), F, dtype=torch.float64, device=dev) if want_hist else None
    status = torch.full((ld,), I, dtype=torch.int32, device=dev); iters = torch.full((ld,), I, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    o = C.byref(opts) if opts is not None else None
    head = (mpc._h, B, ld, steps, p(state), p(coeffs), p(ylo), p(yhi), p(w))
    tail = (p(hist), p(status), p(iters), stream)
    ws = 1 if warm_start else 0
    if kind == "fused" or kind == "fused_null":
        rc = lib.mpc_rollout_batch_device_fused_model(*head, p(md), ws, o, *tail)
    elif kind == "stepwise" or kind == "stepwise_null":
        rc = lib.mpc_rollout_batch_device_warm_model(*head, p(md), o, *tail) if warm_start else lib.mpc_rollout_batch_device_model(*head, p(md), *tail)
    elif kind == "plain_fused":
        rc = lib.mpc_rollout_batch_device_fused(*head, ws, o, *tail)
    else:
        rc = lib.mpc_rollout_batch_device_warm(*head, o, *tail) if warm_start else lib.mpc_rollout_batch_device(*head, *tail)
    assert rc == expect, (rc, lib.mpc_last_error())
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy() if t is not None else None
    return {"hist": n(hist), "state": n(state), "status": n(status), "iters": n(iters)}


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


@pytest.mark.parametrize("B", [193, 7])
def test_warm_model_solve(pkg, fast, pop, twin, torch_dev, B):
    """B = 193 with ld = 256 and B = 7.  warm_in = NULL: bitwise mpc_solve_batch_device_model, and the records are written.  A second
    call from those records, in place, follows the oracle and the CPU build.  Nothing from column B on is written."""
    b, model = _cols(pop["b"], slice(0, B)), np.ascontiguousarray(pop["model"][:, :B])
    opts = pkg.warm_opts_default()
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        cold = _solve(pkg, mpc, b, model, torch_dev, kind="model", ld=256)
        first = _solve(pkg, mpc, b, model, torch_dev, ld=256)
        second = _solve(pkg, mpc, b, model, torch_dev, ld=256, inplace=first["dev"])
        st = mpc.stats()
    assert cold["pad"] and first["pad"] and second["pad"]
    _assert_bitwise(first, cold, "warm_in = NULL, B=%d" % B)
    assert np.isfinite(first["warm"]).all() and np.isfinite(second["warm"]).all()
    wpad = second["dev"]["warm"].cpu().numpy()[:, B:]; spad = second["dev"]["status"].cpu().numpy()[B:]
    assert (wpad == F).all() and (spad == I).all()
    ref = {k: v[..., :B] for k, v in pop["oracle"].items()}
    assert_matches_oracle(second, ref, what="warm model solve B=%d ld=256" % B)
    t1 = twin_warm_model_solve(twin, fast, b, model, opts, want_traj=True)
    t2 = twin_warm_model_solve(twin, fast, b, model, opts, warm=t1["warm"], warm_status=t1["status"], want_traj=True)
    _assert_follows_twin(second, t2, "warm model solve B=%d" % B)
    ok = ref["status"] == 0
    print("B=%d: iterations warm / cold %.3f" % (B, second["iters"][ok].sum() / first["iters"][ok].sum()))
    assert second["iters"][ok].sum() < first["iters"][ok].sum()
    assert st.batch == B and st.n_infeasible == int((ref["status"] == INFEASIBLE).sum()) and st.n_success == int(ok.sum())


def test_narrowed_limit(pkg, fast, pop, torch_dev):
    """The records of a cold call go to a call whose max_steering row is halved: the columns holding a |delta_k| above
    max_steering_i (1 + 1e-8) are bitwise mpc_solve_batch_device_model on the same handle, iterations included; at least 8 of them
    and at least 8 that start warm; all statuses are the cold call's.  All-NaN and far-off records: the cold solve on every column."""
    b, model = pop["b"], pop["model"]
    narrow = model.copy(); narrow[2] *= 0.5
    with pkg.BatchedMPC(fast, 193, device=0) as mpc:
        first = _solve(pkg, mpc, b, model, torch_dev)
        cold = _solve(pkg, mpc, b, narrow, torch_dev, kind="model")
        got = _solve(pkg, mpc, b, narrow, torch_dev, warm=first["warm"], warm_status=first["status"])
        cold_same = _solve(pkg, mpc, b, model, torch_dev, kind="model")
        spoilt = [_solve(pkg, mpc, b, model, torch_dev, warm=g, warm_status=first["status"]) for g in garbage_warm(fast, first["warm"])]
    good = first["status"] == 0
    refused = good & steering_outside(fast.N, first["warm"], narrow[2])
    warm = good & ~refused
    print("halved max_steering: %d records refused, %d start warm, iterations warm / cold on those %.3f" %
          (refused.sum(), warm.sum(), got["iters"][warm].sum() / cold["iters"][warm].sum()))
    assert refused.sum() >= 8 and warm.sum() >= 8
    assert np.array_equal(got["status"], cold["status"])
    for k in KEYS:
        assert np.array_equal(got[k][..., refused], cold[k][..., refused]), k
        assert np.array_equal(got[k][..., ~good], cold[k][..., ~good]), k
    assert got["iters"][warm].sum() < cold["iters"][warm].sum() and (got["iters"][warm] != cold["iters"][warm]).sum() >= 8
    for g in spoilt:
        _assert_bitwise(g, cold_same, "spoilt records")


def test_lane_compaction(pkg, fast, pop, torch_dev):
    """B = 8 256 (compaction runs from 8 192), a warm model call in place: bitwise the same call on a handle with lane_compact = 0."""
    B = 8256
    b = _cols(pop["b"], np.arange(B) % 193)
    model = draw_rows(fast, B, seed=6)
    got = []
    for lc in (fast.lane_compact, 0):
        with pkg.BatchedMPC(_with(fast, lane_compact=lc), B, device=0) as mpc:
            first = _solve(pkg, mpc, b, model, torch_dev)
            got.append((first, _solve(pkg, mpc, b, model, torch_dev, inplace=first["dev"])))
    for k in (0, 1):
        _assert_bitwise(got[0][k], got[1][k], "lane compaction on / off, call %d" % k, keys=KEYS + ("warm",))
    ok = got[0][0]["status"] == 0
    assert np.array_equal(got[0][1]["status"], got[0][0]["status"]) and got[0][1]["iters"][ok].sum() < got[0][0]["iters"][ok].sum()


def test_stepwise_warm_rollout(pkg, fast, pop, torch_dev):
    """64 cars x 6 steps: hist, state, status and iters equal a loop of mpc_solve_batch_device_warm_model calls fed as src/test.cpp
    feeds them (step 1 cold, the buffers in place from then on), and every solve of every 4th car follows the oracle's own loop."""
    B, steps = 64, 6
    cars = np.where(pop["oracle"]["status"] == 0)[0][:B]
    b, model = _cols(pop["b"], cars), np.ascontiguousarray(pop["model"][:, cars])
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        r = _roll(pkg, mpc, b, model, steps, torch_dev, "stepwise", warm_start=True)
        st = mpc.stats()
        cur = dict(b); lh = np.zeros((steps, 9, B)); ls = np.zeros(B, dtype=np.int32); li = np.zeros(B, dtype=np.int32)
        sst = np.zeros((steps, B), dtype=np.int32)
        buf = None
        for k in range(steps):
            g = _solve(pkg, mpc, cur, model, torch_dev, inplace=buf)
            buf = g["dev"]
            lh[k] = g["out"]; sst[k] = g["status"]; ls = np.maximum(ls, g["status"]) if k else g["status"].copy(); li += g["iters"]
            cur = dict(cur, state=g["out"][:6].copy())
        cold = _roll(pkg, mpc, b, model, steps, torch_dev, "stepwise")
    assert np.array_equal(r["hist"], lh) and np.array_equal(r["state"], lh[-1, :6]) and np.array_equal(r["status"], ls) and np.array_equal(r["iters"], li)
    assert st.batch == B and st.n_success == int((r["status"] == 0).sum()) and st.iter_sum == int(li.sum())
    assert_loops_follow_oracle(r["hist"], sst, oracle_model_loops("config-fast.json", b, model, range(0, B, 4), steps), what="stepwise warm rollout")
    print("64 cars x 6 steps: iterations warm / cold %.3f" % (r["iters"].sum() / cold["iters"].sum()))
    assert (r["status"] == 0).all() and r["iters"].sum() < cold["iters"].sum()


SHAPES = {"B1061_ld1088": (1061, 1088, False), "B7": (7, 8, False), "B193_weights": (193, 256, True)}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", list(MODES))
def test_fused_is_stepwise(pkg, fast, waypoints, torch_dev, mode, shape):
    """6 steps, cold, warm and warm with shift = 1; B = 1 061 with ld = 1 088 (17 wavefronts, the last ragged), B = 7 (one partial
    wave, below the wave limit) and B = 193 with per-car weights; with history and without.  hist, state, status and iters are equal,
    mpc_get_stats is equal field for field, mpc_rollout_fused_info counts the fused launches, nothing is written beyond column B - 1."""
    warm_start, o = MODES[mode]
    opts = pkg.warm_opts_default(**o)
    B, ld, with_w = SHAPES[shape]
    steps = 6
    sc, model = population(pkg, fast, waypoints, B) if B == 193 else (pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=61), draw_rows(fast, B))
    sc = {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    w = np.array(list(fast.weights))[:12, None] * (0.5 + np.random.default_rng(122).random(B))[None, :] if with_w else None
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        ref = _roll(pkg, mpc, sc, model, steps, torch_dev, "stepwise", warm_start, opts, weights=w, ld=ld)
        st_ref = mpc.stats()
        assert mpc.rollout_fused_info() == {"fused_launches": 0, "stepwise_loops": 0}
        got = _roll(pkg, mpc, sc, model, steps, torch_dev, "fused", warm_start, opts, weights=w, ld=ld)
        st_got = mpc.stats()
        nohist = _roll(pkg, mpc, sc, model, steps, torch_dev, "fused", warm_start, opts, weights=w, ld=ld, want_hist=False)
        assert mpc.rollout_fused_info() == {"fused_launches": 2, "stepwise_loops": 0}
    assert (ref["status"][:B] != I).all() and (ref["iters"][:B] != I).all() and np.array_equal(ref["state"][:, :B], ref["hist"][-1, :6, :B])
    for k in ("hist", "state", "status", "iters"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), (mode, shape, k)
        if k != "hist":
            assert np.array_equal(nohist[k], ref[k], equal_nan=True), (mode, shape, k, "no history")
    for k in ("hist", "status", "iters"):
        assert (got[k][..., B:] == (I if got[k].dtype == np.int32 else F)).all(), (mode, shape, k, "written beyond column B - 1")
    assert (got["state"][:, B:] == 0).all() and (nohist["status"][B:] == I).all() and (nohist["iters"][B:] == I).all()
    assert np.isfinite(got["hist"][..., :B]).all()
    for f in STAT_FIELDS:
        assert getattr(st_got, f) == getattr(st_ref, f), f
    assert st_got.batch == B and st_got.iter_sum == int(ref["iters"][:B].sum())
    if B > 7:
        assert (ref["status"][:B] == INFEASIBLE).any() and (ref["status"][:B] == 0).any()      # (both kinds of car are there)


def test_default_handle_at_n25(pkg, golden_dir, waypoints, torch_dev):
    """config-stable.json with N = 25, dt = 0.05 and default parameters (f64_f32_start = AUTO: the ordinary solve starts in fp32),
    B = 130, 3 steps: the warm model solve and both fused forms succeed and are bitwise those of a handle with f64_f32_start = 0."""
    p = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"), N=25, dt=0.05)
    assert p.f64_f32_start == 2
    B, steps = 130, 3
    b = pkg.scenarios.lake_track_batch(B, p, waypoints, seed=77)
    b = {k: np.ascontiguousarray(b[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    model = draw_rows(p, B, dts=(0.04, 0.05, 0.06))
    got = []
    for start in (p.f64_f32_start, 0):
        with pkg.BatchedMPC(_with(p, f64_f32_start=start), B, device=0) as mpc:
            first = _solve(pkg, mpc, b, model, torch_dev)
            second = _solve(pkg, mpc, b, model, torch_dev, inplace=first["dev"])
            rolls = [_roll(pkg, mpc, b, model, steps, torch_dev, "fused", ws) for ws in (False, True)]
            step = [_roll(pkg, mpc, b, model, steps, torch_dev, "stepwise", ws) for ws in (False, True)]
            assert mpc.rollout_fused_info() == {"fused_launches": 2, "stepwise_loops": 0}
            got.append((first, second, rolls, step))
    for k in (0, 1):
        _assert_bitwise(got[0][k], got[1][k], "fp32-start handle / fp64 handle, solve %d" % k, keys=KEYS + ("warm",))
        for form in (2, 3):
            for key in ("hist", "state", "status", "iters"):
                assert np.array_equal(got[0][form][k][key], got[1][form][k][key], equal_nan=True), (form, k, key)
        for key in ("hist", "state", "status", "iters"):
            assert np.array_equal(got[0][2][k][key], got[0][3][k][key], equal_nan=True), ("fused / stepwise", k, key)
    ok = got[0][0]["status"] == 0
    assert ok.sum() > B // 2 and np.array_equal(got[0][1]["status"], got[0][0]["status"])
    assert got[0][1]["iters"][ok].sum() < got[0][0]["iters"][ok].sum()


def test_refusals_and_forwarding(pkg, fast, pop, waypoints, torch_dev):
    import torch
    lib = pkg.library()
    # an fp32 handle is refused with the model message, whatever else it is asked
    b1 = _cols(pop["b"], slice(0, 8))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch_dev)
    m = torch.from_numpy(pkg.scenarios.model_rows(fast, 8)).to(torch_dev)
    out = torch.zeros((9, 8), dtype=torch.float32, device=torch_dev); status = torch.zeros(8, dtype=torch.int32, device=torch_dev)
    wb = torch.zeros(((fast.N - 1) * WARM_REC, 8), dtype=torch.float64, device=torch_dev)
    hb = np.zeros(((fast.N - 1) * WARM_REC, 8)); ho = np.zeros((9, 8), dtype=np.float32); hs = np.zeros(8, dtype=np.int32)
    with pkg.BatchedMPC(_with(fast, precision=pkg.PRECISION_F32), 8, device=0) as mpc:
        st, cf, yl, yh = f(b1["state"]), f(b1["coeffs"]), f(b1["yaw_lo"]), f(b1["yaw_hi"])
        head = (st.data_ptr(), cf.data_ptr(), yl.data_ptr(), yh.data_ptr(), None, m.data_ptr())
        hm = pkg.scenarios.model_rows(fast, 8)
        hh = tuple(np.ascontiguousarray(b1[k], dtype=np.float32) for k in ("state", "coeffs", "yaw_lo", "yaw_hi"))
        for call in (lambda: lib.mpc_solve_batch_device_warm_model(mpc._h, 8, 8, *head, None, None, wb.data_ptr(), 8, None, out.data_ptr(), None,
                                                                   status.data_ptr(), None, None),
                     lambda: lib.mpc_solve_batch_host_warm_model(mpc._h, 8, 8, *(a.ctypes.data for a in hh), None, hm.ctypes.data, None, None,
                                                                 hb.ctypes.data, 8, None, ho.ctypes.data, None, hs.ctypes.data, None),
                     lambda: lib.mpc_rollout_batch_device_warm_model(mpc._h, 8, 8, 2, *head, None, None, status.data_ptr(), None, None),
                     lambda: lib.mpc_rollout_batch_device_fused_model(mpc._h, 8, 8, 2, *head, 0, None, None, status.data_ptr(), None, None),
                     lambda: lib.mpc_rollout_batch_device_fused_model(mpc._h, 8, 8, 2, *head, 1, None, None, status.data_ptr(), None, None)):
            assert call() == -1
            assert b"per-instance model values: fp64 handles only" in lib.mpc_last_error()
        torch.cuda.synchronize()
    # the second-order correction: a warm start is refused, and the fused cold call is the stepwise loop
    B, steps = 193, 4
    b, model = pop["b"], pop["model"]
    with pkg.BatchedMPC(_with(fast, max_soc=4), B, device=0) as mpc:
        assert _solve(pkg, mpc, b, model, torch_dev, expect=-4) is None
        assert b"second-order correction" in lib.mpc_last_error()
        _roll(pkg, mpc, b, model, steps, torch_dev, "stepwise", True, expect=-4)
        _roll(pkg, mpc, b, model, steps, torch_dev, "fused", True, expect=-4)
        assert mpc.rollout_fused_info() == {"fused_launches": 0, "stepwise_loops": 0}
        ref = _roll(pkg, mpc, b, model, steps, torch_dev, "stepwise", False)
        got = _roll(pkg, mpc, b, model, steps, torch_dev, "fused", False)
        assert mpc.rollout_fused_info() == {"fused_launches": 0, "stepwise_loops": 1}
    for k in ("hist", "state", "status", "iters"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), ("max_soc = 4", k)
    # model = NULL is the entry point without _model, bitwise: on the wave path (B = 192) and on the lane kernel (B = 1 061)
    opts = pkg.warm_opts_default()
    for B in (192, 1061):
        sc = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=77)
        sc = {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
        with pkg.BatchedMPC(fast, B, device=0) as mpc:
            p1 = _solve(pkg, mpc, sc, None, torch_dev, kind="warm")
            p2 = _solve(pkg, mpc, sc, None, torch_dev, kind="warm", warm=p1["warm"], warm_status=p1["status"])
            f1 = _solve(pkg, mpc, sc, None, torch_dev)
            f2 = _solve(pkg, mpc, sc, None, torch_dev, warm=p1["warm"], warm_status=p1["status"])
            _assert_bitwise(f1, p1, "model = NULL, B = %d" % B, keys=KEYS + ("warm",))
            _assert_bitwise(f2, p2, "model = NULL, warm, B = %d" % B, keys=KEYS + ("warm",))
            hp = mpc.solve_numpy_warm(sc["state"], sc["coeffs"], sc["yaw_lo"], sc["yaw_hi"], warm=p1["warm"], warm_status=p1["status"], want_traj=True)
            hf = {k: np.zeros_like(hp[k]) for k in KEYS + ("warm",)}
            a = lambda x: x.ctypes.data
            assert lib.mpc_solve_batch_host_warm_model(mpc._h, B, B, a(sc["state"]), a(sc["coeffs"]), a(sc["yaw_lo"]), a(sc["yaw_hi"]), None, None,
                                                       a(p1["warm"]), a(p1["status"]), a(hf["warm"]), B, None, a(hf["out"]), a(hf["traj"]),
                                                       a(hf["status"]), a(hf["iters"])) == 0
            _assert_bitwise(hf, hp, "model = NULL, host, B = %d" % B, keys=KEYS + ("warm",))
            before = mpc.rollout_fused_info()
            for ws in (False, True):
                for null_kind, plain_kind in (("stepwise_null", "plain"), ("fused_null", "plain_fused")):
                    x = _roll(pkg, mpc, sc, None, 3, torch_dev, null_kind, ws, opts)
                    y = _roll(pkg, mpc, sc, None, 3, torch_dev, plain_kind, ws, opts)
                    for k in ("hist", "state", "status", "iters"):
                        assert np.array_equal(x[k], y[k], equal_nan=True), (B, ws, null_kind, k)
            after = mpc.rollout_fused_info()
        # (the forwarded fused calls take the path of the plain ones: the wave path's stepwise loop at B = 192, the one launch at 1 061)
        key = "stepwise_loops" if B == 192 else "fused_launches"
        assert after[key] - before[key] == 4


def test_host_entry_point_and_python_arguments(pkg, fast, pop, torch_dev):
    """mpc_solve_batch_host_warm_model (solve_numpy_warm), solve_torch(model=, warm=...) and rollout_torch(model=, warm_start=True,
    fused=True) give the device calls' results, bitwise; a model of the wrong shape is still a ValueError."""
    import torch
    b, model = pop["b"], pop["model"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dev)
    ins = lambda: (t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]))
    keys = KEYS + ("warm",)
    steps = 4
    with pkg.BatchedMPC(fast, 193, device=0) as mpc:
        first = _solve(pkg, mpc, b, model, torch_dev)
        ref = _solve(pkg, mpc, b, model, torch_dev, warm=first["warm"], warm_status=first["status"])
        h1 = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], want_traj=True, model=model)
        h2 = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], warm=h1["warm"], warm_status=h1["status"], want_traj=True, model=model)
        r1 = mpc.solve_torch(*ins(), want_traj=True, want_warm=True, model=t(model))
        r2 = mpc.solve_torch(*ins(), want_traj=True, warm=r1["warm"], warm_status=r1["status"], model=t(model))
        torch.cuda.synchronize()
        d1 = {k: r1[k].cpu().numpy() for k in keys}; d2 = {k: r2[k].cpu().numpy() for k in keys}
        with pytest.raises(ValueError):
            mpc.solve_torch(*ins(), want_warm=True, model=t(model[:5]))
        with pytest.raises(ValueError):
            mpc.rollout_torch(*ins(), steps=2, warm_start=True, fused=True, model=t(model[:, :5]))
        rolls = {}
        for ws in (False, True):
            want = _roll(pkg, mpc, b, model, steps, torch_dev, "stepwise", ws)
            for fused in (False, True):
                state = t(b["state"])
                r = mpc.rollout_torch(state, *ins()[1:], steps=steps, warm_start=ws, fused=fused, model=t(model))
                torch.cuda.synchronize()
                rolls[(ws, fused)] = ({"hist": r["hist"].cpu().numpy(), "state": state.cpu().numpy(), "status": r["status"].cpu().numpy(),
                                       "iters": r["iters"].cpu().numpy()}, want)
        assert mpc.rollout_fused_info() == {"fused_launches": 2, "stepwise_loops": 0}
    _assert_bitwise(h1, first, "host, warm_in = NULL", keys)
    _assert_bitwise(h2, ref, "host, warm", keys)
    _assert_bitwise(d1, first, "solve_torch, want_warm", keys)
    _assert_bitwise(d2, ref, "solve_torch, warm", keys)
    for (ws, fused), (g, want) in rolls.items():
        for k in ("hist", "state", "status", "iters"):
            assert np.array_equal(g[k], want[k], equal_nan=True), (ws, fused, k)
