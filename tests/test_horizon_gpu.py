"""Per-instance horizon on the device (the seven mpc_*_horizon entry points): the HORIZON builds of the lane kernel against
mpc_solve_batch_device_model / the _model rollouts on handles created with N = n_i (bitwise), the oracle with one OrcConfig of
N = n_i per instance, and the stepwise loops the fused call stands for.  Every output array holds sentinels before a call."""
import ctypes as C
import os

import numpy as np
import pytest

from horizon_helpers import (HORIZONS, INFEASIBLE, SENTINEL, WARM_REC, assert_columns_equal_per_n, draw_horizons, judge_n_dt, masked_traj,
                             n_dt_study, oracle_horizon_solve, stated_population, sub_batch, with_N)
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ
from model_helpers import assert_matches_oracle

pytestmark = pytest.mark.gpu

F, I = SENTINEL, -12345          # what the output arrays hold before a call


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pop(pkg, golden_dir, waypoints):
    return stated_population(pkg, golden_dir, waypoints)


def _with(params, **kw):
    p = params.copy()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _wide(a, ld, dev, dtype=np.float64):
    import torch
    a = np.atleast_2d(np.asarray(a, dtype=dtype))
    w = np.zeros((a.shape[0], ld), dtype=dtype); w[:, :a.shape[1]] = a
    return torch.from_numpy(w).to(dev)


def _solve(pkg, mpc, b, dev, horizon=None, model=None, form="horizon", warm_call=False, warm=None, warm_status=None, inplace=None, opts=None,
           weights=None, ld=None, ld_warm=None, expect=0, ld_arg=None, ld_warm_arg=None):
    """One solve through the C ABI, leading dimension ld (default B), sentinels in every output array -> numpy, B columns.
    form: "horizon" (the _horizon / _warm_horizon entry points; horizon may be None = NULL), "model" (the _model / _warm_model ones) or
    "plain" (mpc_solve_batch_device).  inplace: {"warm", "status"} device tensors used as warm_in = warm_out, warm_status = status."""
    import torch
    B = b["state"].shape[1]
    ld = ld or B
    ldw = ld_warm or ld
    N, rows = mpc.N, mpc.warm_rows()
    st, cf, yl, yh = (_wide(b[k], ld, dev) for k in ("state", "coeffs", "yaw_lo", "yaw_hi"))
    md = _wide(model, ld, dev) if model is not None else None
    hz = _wide(horizon, ld, dev, np.int32)[0].contiguous() if horizon is not None else None
    w = _wide(weights, ld, dev) if weights is not None else None
    out = torch.full((9, ld), F, dtype=torch.float64, device=dev)
    tr = torch.full((2 * N, ld), F, dtype=torch.float64, device=dev)
    iters = torch.full((ld,), I, dtype=torch.int32, device=dev)
    wide_w = max(ldw, B)
    if inplace is not None:
        w_in = w_out = inplace["warm"]; w_st = status = inplace["status"]
    else:
        w_in = _wide(warm, wide_w, dev) if warm is not None else None
        w_st = _wide(warm_status, ld, dev, np.int32)[0].contiguous() if warm_status is not None else None
        w_out = torch.full((rows, wide_w), F, dtype=torch.float64, device=dev) if warm_call else None
        status = torch.full((ld,), I, dtype=torch.int32, device=dev)
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None
    o = C.byref(opts) if opts is not None else None
    head = (mpc._h, B, ld if ld_arg is None else ld_arg, p(st), p(cf), p(yl), p(yh), p(w))      # (ld_arg / ld_warm_arg: what the call is told, whatever the arrays' width)
    tail = (p(out), p(tr), p(status), p(iters), stream)
    wa = (p(w_in), p(w_st), p(w_out), ldw if ld_warm_arg is None else ld_warm_arg, o)
    if form == "plain":
        rc = lib.mpc_solve_batch_device(*head, *tail)
    elif form == "model":
        rc = lib.mpc_solve_batch_device_warm_model(*head, p(md), *wa, *tail) if warm_call else lib.mpc_solve_batch_device_model(*head, p(md), *tail)
    else:
        rc = (lib.mpc_solve_batch_device_warm_horizon(*head, p(md), p(hz), *wa, *tail) if warm_call else
              lib.mpc_solve_batch_device_horizon(*head, p(md), p(hz), *tail))
    assert rc == expect, (rc, lib.mpc_last_error())
    torch.cuda.synchronize()
    if expect:
        return lib.mpc_last_error().decode()
    o_, t_, s_, it_ = (x.cpu().numpy() for x in (out, tr, status, iters))
    wm = w_out.cpu().numpy() if w_out is not None else None
    pad = bool((o_[:, B:] == F).all() and (t_[:, B:] == F).all() and (it_[B:] == I).all())
    return {"out": o_[:, :B].copy(), "traj": t_[:, :B].copy(), "status": s_[:B].copy(), "iters": it_[:B].copy(),
            "warm": wm[:, :B].copy() if wm is not None else None, "pad": pad, "dev": {"warm": w_out, "status": status}}


@pytest.fixture(scope="module")
def per_n(pkg, pop, dev):
    """The yardstick, computed once and left unchanged: for every horizon n of the stated set, the 193 instances through
    mpc_solve_batch_device_model and _warm_model (cold, then warm from it with shift 0 and 1) on a handle created with N = n and
    f64_f32_start = 0."""
    params, b, model, _ = pop
    res = {}
    for n in HORIZONS:
        with pkg.BatchedMPC(_with(with_N(params, n), f64_f32_start=0), 256, device=0) as mpc:
            cold = _solve(pkg, mpc, b, dev, model=model, form="model", warm_call=True)
            res[n] = {"cold": cold}
            for shift in (0, 1):
                res[n]["warm%d" % shift] = _solve(pkg, mpc, b, dev, model=model, form="model", warm_call=True, warm=cold["warm"],
                                                  warm_status=cold["status"], opts=pkg.warm_opts_default(shift=shift))
    return res


def _ref(per_n, key):
    return lambda n, idx: {k: (v[..., idx] if isinstance(v, np.ndarray) else v) for k, v in per_n[n][key].items() if k in ("out", "traj", "status", "iters", "warm")}


def _layouts(horizon):
    B = horizon.shape[0]
    one3 = horizon.copy(); one3[64:128] = 3
    mixed = one3.copy(); mixed[64 + 37] = 25
    return {"shuffled": horizon, "sorted": np.sort(horizon), "a wave of 3": one3, "a wave of 3 with one lane of 25": mixed}


@pytest.mark.parametrize("f32_start", (0, 2))
def test_columns_are_those_of_handles_of_that_N_bitwise(pkg, pop, per_n, dev, f32_start):
    """193 instances (three full waves and one lane) on an N = 25 handle, four layouts of the horizons, cold and warm: every column
    is mpc_solve_batch_device_model's / _warm_model's on a handle created with N = n_i, sentinels behind the prefixes.  f32_start 2
    is the default N = 25 handle, whose ordinary solve starts in fp32."""
    params, b, model, horizon = pop
    with pkg.BatchedMPC(_with(params, f64_f32_start=f32_start), 256, device=0) as mpc:
        for name, hz in _layouts(horizon).items():
            cold = _solve(pkg, mpc, b, dev, hz, model, warm_call=True)
            assert cold["pad"], name
            assert_columns_equal_per_n(cold, params.N, hz, _ref(per_n, "cold"), name)
            nowarm = _solve(pkg, mpc, b, dev, hz, model)                       # (the cold entry point: the same bits, no warm_out)
            for k in ("out", "traj", "status", "iters"):
                assert np.array_equal(nowarm[k], cold[k], equal_nan=True), (name, k)
            if name in ("shuffled", "a wave of 3 with one lane of 25"):
                for shift in (0, 1):
                    warm = _solve(pkg, mpc, b, dev, hz, model, warm_call=True, warm=cold["warm"], warm_status=cold["status"],
                                  opts=pkg.warm_opts_default(shift=shift))
                    assert_columns_equal_per_n(warm, params.N, hz, _ref(per_n, "warm%d" % shift), "%s warm shift %d" % (name, shift))


def test_one_instance_and_a_wider_leading_dimension(pkg, pop, per_n, dev):
    params, b, model, horizon = pop
    with pkg.BatchedMPC(params, 256, device=0) as mpc:
        for i in (0, 77):
            one = _solve(pkg, mpc, sub_batch(b, [i]), dev, horizon[[i]], model[:, [i]], warm_call=True)
            assert_columns_equal_per_n(one, params.N, horizon[[i]], lambda n, idx: _ref(per_n, "cold")(n, np.array([i])), "B = 1")
        wide = _solve(pkg, mpc, b, dev, horizon, model, warm_call=True, ld=200, ld_warm=208)
        assert wide["pad"] and (wide["dev"]["warm"].cpu().numpy()[:, 193:] == F).all()
        assert_columns_equal_per_n(wide, params.N, horizon, _ref(per_n, "cold"), "ld > B")


def test_no_model_uses_the_handles_values(pkg, pop, dev):
    """model = NULL with a horizon: bitwise the plain solve of a handle created with N = n (f64_f32_start = 0, no wave path)."""
    params, b, _, horizon = pop
    hz = np.where(horizon > 10, 10, horizon).astype(np.int32)
    with pkg.BatchedMPC(with_N(params, 10), 256, device=0) as mpc:
        got = _solve(pkg, mpc, b, dev, hz, None)

    def ref_of(n, idx):
        with pkg.BatchedMPC(_with(with_N(params, n), f64_f32_start=0, wave_max_batch=-1), 256, device=0) as m:
            return _solve(pkg, m, sub_batch(b, idx), dev, form="plain")
    assert_columns_equal_per_n(got, 10, hz, ref_of, "no model")


def test_lane_compaction_changes_nothing(pkg, golden_dir, waypoints, dev):
    """B = 8 256 on an N = 10 handle, horizons from {3, 5, 10} shuffled: the call with lane compaction against lane_compact = 0."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    B = 8256
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=77)
    b = {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    hz = draw_horizons(B, seed=11, choices=(3, 5, 10))
    res = {}
    for lc in (-1, 0):
        with pkg.BatchedMPC(_with(params, lane_compact=lc), B, device=0) as mpc:
            res[lc] = _solve(pkg, mpc, b, dev, hz, None, warm_call=True)
    for k in ("out", "traj", "status", "iters", "warm"):
        assert np.array_equal(res[-1][k], res[0][k], equal_nan=True), k
    assert (res[0]["status"] == 0).sum() > 0.9 * B


def test_every_instance_against_the_oracle(pkg, pop, dev):
    params, b, model, horizon = pop
    ref = oracle_horizon_solve("config-fast.json", b, model, horizon, params.N)
    with pkg.BatchedMPC(params, 256, device=0) as mpc:
        got = _solve(pkg, mpc, b, dev, horizon, model)
    assert_matches_oracle(masked_traj(got, params.N, horizon), ref, what="device, per-instance horizon")


def test_warm_rules(pkg, pop, dev):
    """In place equals separate buffers; only SUCCESS columns start warm; a record that no longer fits starts cold, bitwise."""
    params, b, model, horizon = pop
    opts = pkg.warm_opts_default()
    with pkg.BatchedMPC(params, 256, device=0) as mpc:
        cold = _solve(pkg, mpc, b, dev, horizon, model, warm_call=True)
        sep = _solve(pkg, mpc, b, dev, horizon, model, warm_call=True, warm=cold["warm"], warm_status=cold["status"], opts=opts)
        first = _solve(pkg, mpc, b, dev, horizon, model, warm_call=True)
        inp = _solve(pkg, mpc, b, dev, horizon, model, warm_call=True, inplace=first["dev"], opts=opts)
        for k in ("out", "traj", "status", "iters"):
            assert np.array_equal(inp[k], sep[k], equal_nan=True), k
        wi = first["dev"]["warm"].cpu().numpy()[:, :193]
        for i, n in enumerate(horizon):
            r = (int(n) - 1) * WARM_REC
            assert np.array_equal(wi[:r, i], sep["warm"][:r, i], equal_nan=True) and (wi[r:, i] == F).all(), i
        ok = cold["status"] == 0
        assert sep["iters"][ok].sum() < cold["iters"][ok].sum()
        for k in ("out", "status", "iters"):
            assert np.array_equal(sep[k][..., ~ok], cold[k][..., ~ok], equal_nan=True), k
        # every status says SUCCESS, but the records of two columns no longer fit (a delta far outside the box, a NaN): they start
        # cold and are bitwise the cold call, iterations included
        spoilt = cold["warm"].copy()
        far, nan = np.nonzero(ok)[0][:2]
        spoilt[6, far] = 1e3; spoilt[0, nan] = np.nan
        got = _solve(pkg, mpc, b, dev, horizon, model, warm_call=True, warm=spoilt, warm_status=np.zeros(193, dtype=np.int32), opts=opts)
        for i in (far, nan):
            for k in ("out", "traj", "status", "iters"):
                assert np.array_equal(got[k][..., i], cold[k][..., i], equal_nan=True), (i, k)
        # a record written under a LONGER horizon is an ordinary candidate under a shorter one: its first n - 1 stages are read and
        # nothing behind them; where the cold solve of the shorter horizon and the warm one both succeed they end at the same point
        # (the stated fp64 tolerances), and a column that was not SUCCESS starts cold, bitwise
        shorter = np.maximum(horizon - 1, 3).astype(np.int32)
        again = _solve(pkg, mpc, b, dev, shorter, model, warm_call=True, warm=cold["warm"], warm_status=cold["status"], opts=opts)
        ref = _solve(pkg, mpc, b, dev, shorter, model, warm_call=True)
        for k in ("out", "status", "iters"):
            assert np.array_equal(again[k][..., ~ok], ref[k][..., ~ok], equal_nan=True), k
        both = (again["status"] == 0) & (ref["status"] == 0)
        assert both.sum() > 150
        d = np.abs(again["out"][:, both] - ref["out"][:, both])
        assert d[6].max() <= TOL_STEER and d[7].max() <= TOL_ACCEL and d[:6].max() <= TOL_TRAJ, (d[6].max(), d[7].max(), d[:6].max())


def _roll(pkg, mpc, sc, dev, steps, horizon, model, kind, warm_start, form="horizon", weights=None, want_hist=True):
    import torch
    B = sc["state"].shape[1]
    state, coeffs, ylo, yhi = (_wide(sc[k], B, dev) for k in ("state", "coeffs", "yaw_lo", "yaw_hi"))
    md = _wide(model, B, dev) if model is not None else None
    hz = _wide(horizon, B, dev, np.int32)[0].contiguous() if horizon is not None else None
    w = _wide(weights, B, dev) if weights is not None else None
    hist = torch.full((steps, 9, B), F, dtype=torch.float64, device=dev) if want_hist else None
    status = torch.full((B,), I, dtype=torch.int32, device=dev); iters = torch.full((B,), I, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (mpc._h, B, B, steps, p(state), p(coeffs), p(ylo), p(yhi), p(w), p(md)) + ((p(hz),) if form == "horizon" else ())
    tail = (p(hist), p(status), p(iters), stream)
    sfx = "_horizon" if form == "horizon" else "_model"
    if kind == "fused":
        rc = getattr(lib, "mpc_rollout_batch_device_fused" + sfx)(*head, 1 if warm_start else 0, None, *tail)
    elif warm_start:
        rc = getattr(lib, "mpc_rollout_batch_device_warm" + sfx)(*head, None, *tail)
    else:
        rc = getattr(lib, "mpc_rollout_batch_device" + sfx)(*head, *tail)
    assert rc == 0, (rc, lib.mpc_last_error())
    torch.cuda.synchronize()
    return {"hist": hist.cpu().numpy() if want_hist else None, "state": state.cpu().numpy(), "status": status.cpu().numpy(), "iters": iters.cpu().numpy()}


def test_rollouts(pkg, golden_dir, waypoints, dev):
    """96 cars x 6 steps on an N = 25 handle, horizons from {3, 5, 10}: the fused form equals the stepwise form bitwise, cold and warm;
    every car equals its car on a handle created with N = n (the _model rollouts); mpc_rollout_fused_info shows the fused launches."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"), N=25)
    cars, steps = 96, 6
    sc = pkg.scenarios.lake_track_batch(cars, params, waypoints, seed=122)
    sc = {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    hz = draw_horizons(cars, seed=11, choices=(3, 5, 10))
    model = pkg.scenarios.model_rows(params, cars); model[0] = np.where(np.arange(cars) % 2, 0.1, 0.08)
    got = {}
    with pkg.BatchedMPC(params, 128, device=0) as mpc:
        for warm_start in (False, True):
            step = _roll(pkg, mpc, sc, dev, steps, hz, model, "stepwise", warm_start)
            before = mpc.rollout_fused_info()
            fused = _roll(pkg, mpc, sc, dev, steps, hz, model, "fused", warm_start)
            after = mpc.rollout_fused_info()
            assert after["fused_launches"] == before["fused_launches"] + 1 and after["stepwise_loops"] == before["stepwise_loops"]
            for k in ("hist", "state", "status", "iters"):
                assert np.array_equal(fused[k], step[k], equal_nan=True), (warm_start, k)
            got[warm_start] = fused
        nohist = _roll(pkg, mpc, sc, dev, steps, hz, model, "fused", True, want_hist=False)
        for k in ("state", "status", "iters"):
            assert np.array_equal(nohist[k], got[True][k], equal_nan=True), k
    assert got[True]["iters"].sum() < got[False]["iters"].sum()
    for n in (3, 5, 10):
        idx = np.nonzero(hz == n)[0]
        with pkg.BatchedMPC(_with(with_N(params, n), f64_f32_start=0), 128, device=0) as mpc:
            for warm_start in (False, True):
                ref = _roll(pkg, mpc, sub_batch(sc, idx), dev, steps, None, model[:, idx], "stepwise", warm_start, form="model")
                for k in ("hist", "state", "status", "iters"):
                    assert np.array_equal(got[warm_start][k][..., idx], ref[k], equal_nan=True), (n, warm_start, k)


def test_the_reference_n_dt_study_in_one_fused_launch(pkg, golden_dir, dev):
    """The 14 N / dt figures of the reference as ONE fused rollout launch on an N = 50 handle: B = 14, 26 steps, judged as the CPU
    test judges."""
    entries, params, sc, W, model, horizon, pre = n_dt_study(pkg, golden_dir)
    with pkg.BatchedMPC(params, 16, device=0) as mpc:
        r = _roll(pkg, mpc, sc, dev, 26, horizon, model, "fused", False, weights=W)
        info = mpc.rollout_fused_info()
    assert info == {"fused_launches": 1, "stepwise_loops": 0}
    judge_n_dt(entries, r["hist"], r["status"], pre)


@pytest.mark.parametrize("B", (16, 2048))
def test_a_null_horizon_is_the_model_form_bitwise(pkg, golden_dir, waypoints, dev, B):
    """horizon = NULL: with `model` the _model form, without it the plain form -- at B = 16 its wave path -- cold and warm."""
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=77)
    b = {k: np.ascontiguousarray(sc[k], dtype=np.float64) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
    model = pkg.scenarios.model_rows(params, B); model[0] = 0.08
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        for md in (model, None):
            for warm_call in (False, True):
                a = _solve(pkg, mpc, b, dev, None, md, warm_call=warm_call)
                r = _solve(pkg, mpc, b, dev, None, md, form="model", warm_call=warm_call)
                for k in ("out", "traj", "status", "iters", "warm"):
                    assert (a[k] is None and r[k] is None) or np.array_equal(a[k], r[k], equal_nan=True), (md is None, warm_call, k)
        plain = _solve(pkg, mpc, b, dev, form="plain")
        null = _solve(pkg, mpc, b, dev, None, None)
        for k in ("out", "traj", "status", "iters"):
            assert np.array_equal(null[k], plain[k], equal_nan=True), k


def test_unusable_horizons(pkg, pop, dev):
    params, b, model, horizon = pop
    bad = {5: 2, 64: 0, 100: -1, 192: params.N + 1}
    hz = horizon.copy()
    for i, v in bad.items():
        hz[i] = v
    with pkg.BatchedMPC(params, 256, device=0) as mpc:
        good = _solve(pkg, mpc, b, dev, horizon, model, warm_call=True)
        got = _solve(pkg, mpc, b, dev, hz, model, warm_call=True)
    at = np.array(sorted(bad)); keep = np.setdiff1d(np.arange(193), at)
    assert (got["status"][at] == INFEASIBLE).all() and np.isfinite(got["out"]).all()
    for k in ("out", "traj", "status", "iters", "warm"):
        assert np.array_equal(got[k][..., keep], good[k][..., keep], equal_nan=True), k


def test_refusals(pkg, pop, dev):
    params, b, model, horizon = pop
    with pkg.BatchedMPC(_with(params, precision=pkg.PRECISION_F32), 256, device=0) as mpc:
        msg = _solve(pkg, mpc, b, dev, horizon, None, expect=-1)
        assert "fp64 handles only" in msg
    with pkg.BatchedMPC(_with(params, max_soc=4), 256, device=0) as mpc:
        msg = _solve(pkg, mpc, b, dev, horizon, model, expect=-4)
        assert "horizon" in msg and "max_soc" in msg
        ok = _solve(pkg, mpc, b, dev, None, model)                    # horizon = NULL: nothing changes, max_soc is honoured
        ref = _solve(pkg, mpc, b, dev, None, model, form="model")
        assert np.array_equal(ok["out"], ref["out"], equal_nan=True)
    with pkg.BatchedMPC(params, 256, device=0) as mpc:
        assert "ld < B" in _solve(pkg, mpc, b, dev, horizon, model, ld_arg=192, expect=-1)
        assert "ld_warm < B" in _solve(pkg, mpc, b, dev, horizon, model, warm_call=True, ld_warm_arg=192, expect=-1)
        again = _solve(pkg, mpc, b, dev, horizon, model)              # (a refused call leaves the handle usable)
        assert (again["status"] == 0).sum() > 150


def test_host_forms_and_the_python_layer(pkg, pop, per_n, dev):
    """mpc_solve_batch_host_horizon / _host_warm_horizon through solve_numpy / solve_numpy_warm: the device forms' bits; the rows of
    traj and warm_out that an instance does not write come back as the caller has them (also with warm_in = warm_out); and
    solve_torch / rollout_torch take `horizon`."""
    import torch
    params, b, model, horizon = pop
    N, rows = params.N, (params.N - 1) * WARM_REC
    with pkg.BatchedMPC(params, 256, device=0) as mpc:
        traj = np.full((2 * N, 193), F)
        cold = mpc.solve_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], model=model, horizon=horizon, traj_out=traj)
        assert cold["traj"] is traj
        assert_columns_equal_per_n(cold, N, horizon, _ref(per_n, "cold"), "solve_numpy")
        wout = np.full((rows, 193), F)
        c2 = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], model=model, horizon=horizon, traj_out=np.full((2 * N, 193), F),
                                  warm_out=wout)
        assert_columns_equal_per_n(c2, N, horizon, _ref(per_n, "cold"), "solve_numpy_warm, cold")
        for shift in (0, 1):
            w2 = np.full((rows, 193), F)
            warm = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], warm=c2["warm"], warm_status=c2["status"], model=model,
                                        horizon=horizon, traj_out=np.full((2 * N, 193), F), warm_out=w2, warm_opts=pkg.warm_opts_default(shift=shift))
            assert_columns_equal_per_n(warm, N, horizon, _ref(per_n, "warm%d" % shift), "solve_numpy_warm, shift %d" % shift)
        inplace = c2["warm"].copy()                      # warm_in = warm_out: the sentinels behind the records stay
        warm = mpc.solve_numpy_warm(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], warm=inplace, warm_status=c2["status"], model=model,
                                    horizon=horizon, traj_out=np.full((2 * N, 193), F), warm_out=inplace)
        assert warm["warm"] is inplace
        assert_columns_equal_per_n(warm, N, horizon, _ref(per_n, "warm0"), "solve_numpy_warm, in place")
        plain = mpc.solve_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], model=model, horizon=horizon, want_traj=True)
        assert np.array_equal(np.isnan(plain["traj"]), traj == F)      # (no traj_out: NaN where nothing is written)
        t = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
        r = mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), model=t(model), horizon=t(horizon, np.int32))
        torch.cuda.synchronize()
        assert np.array_equal(r["out"].cpu().numpy(), cold["out"], equal_nan=True) and np.array_equal(r["status"].cpu().numpy(), cold["status"])
        with pytest.raises(ValueError):
            mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), horizon=t(horizon))      # (float64: refused)
        hz = np.where(horizon > 10, 10, horizon).astype(np.int32)
        res = {}
        for fused in (False, True):
            st = t(b["state"])
            ro = mpc.rollout_torch(st, t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), steps=4, warm_start=True, fused=fused, model=t(model),
                                   horizon=t(hz, np.int32))
            torch.cuda.synchronize()
            res[fused] = [ro["hist"].cpu().numpy(), ro["status"].cpu().numpy(), ro["iters"].cpu().numpy(), st.cpu().numpy()]
        for x, y in zip(res[False], res[True]):
            assert np.array_equal(x, y, equal_nan=True)
        assert mpc.rollout_fused_info() == {"fused_launches": 1, "stepwise_loops": 0}
