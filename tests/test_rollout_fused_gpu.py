"""The fused rollout on the device (mpc_rollout_batch_device_fused: the ROLL builds of the lane kernel, one launch for all steps)
against the stepwise entry points it stands for.  "Equal" is np.array_equal on hist, the final state, status and iters; both forms
run on the same handle from copies of the same inputs."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from helpers import TOL_ACCEL, TOL_STEER, TOL_TRAJ, closed_loop_report

pytestmark = pytest.mark.gpu

F, I = -7777.25, -12345          # what the output arrays hold before a call


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fast(pkg, golden_dir):
    return pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))


def _roll(pkg, mpc, sc, steps, dev, fused, warm_start=False, opts=None, weights=None, want_hist=True, ld=None, expect=0):
    """One rollout through the C ABI with leading dimension ld (default B): the fused entry point, or the stepwise one it stands for.
    Returns hist [steps, 9, ld] (None without history), state [6, ld], status and iters [ld] as numpy -- all ld columns -- or, when the
    call is expected to be refused, its return code."""
    import torch
    B = sc["state"].shape[1]
    ld = ld or B

    def wide(a):
        a = np.atleast_2d(np.asarray(a, dtype=np.float64))
        w = np.zeros((a.shape[0], ld)); w[:, :B] = a
        return torch.from_numpy(w).to(dev)
    state, coeffs, ylo, yhi = wide(sc["state"]), wide(sc["coeffs"]), wide(sc["yaw_lo"]), wide(sc["yaw_hi"])
    w = wide(weights) if weights is not None else None
    hist = torch.full((steps, 9, ld), F, dtype=torch.float64, device=dev) if want_hist else None
    status = torch.full((ld,), I, dtype=torch.int32, device=dev); iters = torch.full((ld,), I, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    lib = pkg.library()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    o = C.byref(opts) if opts is not None else None
    head = (mpc._h, B, ld, steps, p(state), p(coeffs), p(ylo), p(yhi), p(w))
    tail = (p(hist), p(status), p(iters), stream)
    if fused:
        rc = lib.mpc_rollout_batch_device_fused(*head, 1 if warm_start else 0, o, *tail)
    elif warm_start:
        rc = lib.mpc_rollout_batch_device_warm(*head, o, *tail)
    else:
        rc = lib.mpc_rollout_batch_device(*head, *tail)
    assert rc == expect, (rc, lib.mpc_last_error())
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy() if t is not None else None
    return {"hist": n(hist), "state": n(state), "status": n(status), "iters": n(iters)}


def _assert_equal(a, b, what, hist=True):
    for k in ("hist", "state", "status", "iters"):
        if k == "hist" and not hist:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


MODES = {"cold": (False, {}), "warm": (True, {}), "warm_shift1": (True, {"shift": 1})}


@pytest.mark.parametrize("mode", list(MODES))
def test_small_ragged_batch(pkg, fast, waypoints, torch_dev, mode):
    """B = 1061 (above the wave limit: 17 wavefronts, 37 lanes in the last), 6 steps: with history, without, and with ld = 1088 > B."""
    warm_start, o = MODES[mode]
    opts = pkg.warm_opts_default(**o)
    B, steps, ld = 1061, 6, 1088
    sc = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=61)
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        ref = _roll(pkg, mpc, sc, steps, torch_dev, False, warm_start, opts)
        st_ref = mpc.stats()
        ref_ld = _roll(pkg, mpc, sc, steps, torch_dev, False, warm_start, opts, ld=ld)
        assert mpc.rollout_fused_info() == {"fused_launches": 0, "stepwise_loops": 0}
        got = _roll(pkg, mpc, sc, steps, torch_dev, True, warm_start, opts)
        st_got = mpc.stats()
        nohist = _roll(pkg, mpc, sc, steps, torch_dev, True, warm_start, opts, want_hist=False)
        got_ld = _roll(pkg, mpc, sc, steps, torch_dev, True, warm_start, opts, ld=ld)
        assert mpc.rollout_fused_info() == {"fused_launches": 3, "stepwise_loops": 0}
    assert (ref["status"] != I).all() and (ref["iters"] != I).all() and np.array_equal(ref["state"], ref["hist"][-1, :6])
    _assert_equal(got, ref, mode)
    _assert_equal(nohist, ref, mode + ", no history", hist=False)
    _assert_equal(got_ld, ref_ld, mode + ", ld > B")
    for k in ("hist", "status", "iters"):
        assert (got_ld[k][..., B:] == (I if got_ld[k].dtype == np.int32 else F)).all(), (mode, k, "written beyond column B - 1")
        assert np.array_equal(got_ld[k][..., :B], ref[k], equal_nan=True), (mode, k)
    assert (got_ld["state"][:, B:] == 0).all()
    for f in ("batch", "n_success", "n_maxiter", "n_linesearch", "n_infeasible", "n_numeric", "n_acceptable", "iter_sum", "iter_max", "n_pending"):
        assert getattr(st_got, f) == getattr(st_ref, f), f
    assert st_got.batch == B and st_got.iter_sum == int(ref["iters"].sum())


@pytest.fixture(scope="module")
def full_length(pkg, fast, waypoints):
    B = 4096
    sc = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=122)
    scale = 0.5 + np.random.default_rng(122).random(B)
    weights = np.array(list(fast.weights))[:12, None] * scale[None, :]
    return sc, weights


@pytest.mark.parametrize("mode", ["cold", "warm", "warm_weights"])
def test_full_length_loops(pkg, fast, full_length, torch_dev, mode):
    """B = 4096, 25 steps.  The cold population holds cars with a solve that does not succeed: the step after it starts cold in the
    warm rollout, and the status fold has something to fold."""
    sc, weights = full_length
    warm_start = mode != "cold"
    w = weights if mode == "warm_weights" else None
    B, steps = 4096, 25
    opts = pkg.warm_opts_default()
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        ref = _roll(pkg, mpc, sc, steps, torch_dev, False, warm_start, opts, weights=w)
        got = _roll(pkg, mpc, sc, steps, torch_dev, True, warm_start, opts, weights=w)
        assert mpc.rollout_fused_info() == {"fused_launches": 1, "stepwise_loops": 0}
    print(mode, "cars whose worst status is not SUCCESS: %d, iterations per solve %.2f, per car max %d mean %.1f" % (
        (ref["status"] != 0).sum(), ref["iters"].mean() / steps, ref["iters"].max(), ref["iters"].mean()))
    _assert_equal(got, ref, mode)
    if mode == "cold":
        assert (ref["status"] != 0).any()


def test_cars_tiled_over_many_waves(pkg, fast, waypoints, torch_dev):
    """The 96 cars of seed 122 tiled to 4096: every copy of a car is the same car, and the loops are the oracle's."""
    cars, B, steps = 96, 4096, 25
    sc96 = pkg.scenarios.lake_track_batch(cars, fast, waypoints, seed=122)
    idx = np.arange(B) % cars
    sc = {"state": sc96["state"][:, idx], "coeffs": sc96["coeffs"][:, idx], "yaw_lo": sc96["yaw_lo"][idx], "yaw_hi": sc96["yaw_hi"][idx]}
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    _, oh, ost = O.rollout_chunk_full(("config-fast.json", {}, c(sc96["state"]), c(sc96["coeffs"]), c(sc96["yaw_lo"]), c(sc96["yaw_hi"]), steps))
    assert (ost == 0).all()
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        for warm_start in (False, True):
            got = _roll(pkg, mpc, sc, steps, torch_dev, True, warm_start)
            for k in ("hist", "state", "status", "iters"):
                first = got[k][..., :cars]
                for t in range(1, B // cars):
                    assert np.array_equal(got[k][..., t * cars:(t + 1) * cars], first, equal_nan=True), (warm_start, k, t)
                assert np.array_equal(got[k][..., -(B % cars):], first[..., :B % cars], equal_nan=True), (warm_start, k)
            # the call reports a car's worst status: all SUCCESS means every solve succeeded, which is what the oracle says of every solve
            assert (got["status"] == 0).all(), warm_start
            cl = closed_loop_report(got["hist"][:, :, :cars], np.zeros((steps, cars), dtype=np.int32), oh, ost)
            print("fused, warm_start", warm_start, "max |d steer| %.3g |d accel| %.3g |d state| %.3g" % (cl["d_steer_rad"][3], cl["d_accel"][3], cl["d_state"][3]))
            assert cl["status_differs"] == 0 and cl["cars_on_another_local_minimum"] == 0, (warm_start, cl)
            assert cl["d_steer_rad"][3] <= TOL_STEER and cl["d_accel"][3] <= TOL_ACCEL and cl["d_state"][3] <= TOL_TRAJ, (warm_start, cl)
        assert mpc.rollout_fused_info() == {"fused_launches": 2, "stepwise_loops": 0}


def test_stepwise_fallbacks(pkg, fast, waypoints, torch_dev):
    """Where the stepwise loop is not a launch of the single-phase lane kernel per step, the fused call is that loop: a batch on the
    wave path, a handle whose solve starts in fp32, a handle with the second-order correction -- equal, and counted as stepwise."""
    import torch
    steps = 4
    q1 = fast.copy(); q1.f64_f32_start = 1
    q2 = fast.copy(); q2.max_soc = 4
    for name, params, B, warm_modes in (("wave path", fast, 192, (False, True)), ("fp32 start", q1, 1061, (False,)), ("soc", q2, 1061, (False,))):
        sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=61)
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            refs = {}
            for warm_start in warm_modes:
                refs[warm_start] = _roll(pkg, mpc, sc, steps, torch_dev, False, warm_start)
                got = _roll(pkg, mpc, sc, steps, torch_dev, True, warm_start)
                _assert_equal(got, refs[warm_start], (name, warm_start))
                assert (got["status"] != I).all()
            # ... and through the Python handle
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dev)
            r = mpc.rollout_torch(t(sc["state"]), t(sc["coeffs"]), t(sc["yaw_lo"]), t(sc["yaw_hi"]), steps=steps, fused=True)
            torch.cuda.synchronize()
            assert np.array_equal(r["hist"].cpu().numpy(), refs[False]["hist"], equal_nan=True), name
            assert mpc.rollout_fused_info() == {"fused_launches": 0, "stepwise_loops": len(warm_modes) + 1}, name


def test_python_handle_runs_the_fused_kernel(pkg, fast, waypoints, torch_dev):
    import torch
    B, steps = 1061, 3
    sc = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=61)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dev)
    args = lambda: (t(sc["state"]), t(sc["coeffs"]), t(sc["yaw_lo"]), t(sc["yaw_hi"]))
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        for warm_start in (False, True):
            a, b = args(), args()
            ref = mpc.rollout_torch(*a, steps=steps, warm_start=warm_start)
            got = mpc.rollout_torch(*b, steps=steps, warm_start=warm_start, fused=True)
            torch.cuda.synchronize()
            assert torch.equal(a[0], b[0])
            for k in ("hist", "status", "iters"):
                assert np.array_equal(ref[k].cpu().numpy(), got[k].cpu().numpy(), equal_nan=True), (warm_start, k)
        assert mpc.rollout_fused_info() == {"fused_launches": 2, "stepwise_loops": 0}


def test_refusals(pkg, fast, torch_dev):
    """warm_start = 1 on the handles of test_warm_start_gpu.test_refusals: the codes and texts of mpc_rollout_batch_device_warm."""
    import torch
    B = 64
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=torch_dev)
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device=torch_dev)
    lib = pkg.library()

    def both(mpc, opts):
        o = C.byref(opts) if opts is not None else None
        res = []
        for fused in (False, True):
            head = (mpc._h, B, B, 2, z(6, B).data_ptr(), z(5, B).data_ptr(), z(B).data_ptr(), z(B).data_ptr(), None)
            tail = (None, zi(B).data_ptr(), None, None)
            lib.mpc_internal_set_error(b"")
            rc = lib.mpc_rollout_batch_device_fused(*head, 1, o, *tail) if fused else lib.mpc_rollout_batch_device_warm(*head, o, *tail)
            res.append((rc, lib.mpc_last_error()))
        assert res[0] == res[1], res
        return res[1]
    bad = pkg.warm_opts_default(); bad.size = 8
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        rc, msg = both(mpc, bad)
        assert rc == -1 and b"MpcWarmOpts.size" in msg
        bad = pkg.warm_opts_default(); bad.mu_init = 1.0
        assert both(mpc, bad)[0] == -1
    q = fast.copy(); q.precision = pkg.PRECISION_F32
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        rc, msg = both(mpc, None)
        assert rc == -1 and b"fp64 handles only" in msg
    q = fast.copy(); q.max_soc = 4
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        rc, msg = both(mpc, None)
        assert rc == -4 and b"max_soc" in msg
    q = fast.copy(); q.f64_f32_start = 1
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        rc, msg = both(mpc, None)
        assert rc == -4 and b"f64_f32_start" in msg
        with pytest.raises(pkg.MpcError):
            mpc.rollout_torch(z(6, B), z(5, B), z(B), z(B), steps=2, warm_start=True, fused=True)
        assert mpc.rollout_fused_info() == {"fused_launches": 0, "stepwise_loops": 0}


def test_argument_checks(pkg, fast, waypoints, torch_dev):
    import torch
    B = 1061
    sc = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=61)
    lib = pkg.library()
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        for warm_start in (False, True):
            _roll(pkg, mpc, sc, 0, torch_dev, True, warm_start, expect=-1)
            big = {k: np.concatenate([v, v], axis=-1) for k, v in sc.items() if k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
            _roll(pkg, mpc, big, 2, torch_dev, True, warm_start, expect=-1)          # B > max_batch
            st = torch.zeros(B, dtype=torch.int32, device=torch_dev)
            z = torch.zeros((6, B), dtype=torch.float64, device=torch_dev)
            assert lib.mpc_rollout_batch_device_fused(mpc._h, B, B, 2, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, int(warm_start), None, None,
                                                      st.data_ptr(), None, None) == -1
            assert lib.mpc_rollout_batch_device_fused(mpc._h, B, B - 1, 2, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, int(warm_start), None,
                                                      None, st.data_ptr(), None, None) == -1
        assert mpc.rollout_fused_info() == {"fused_launches": 0, "stepwise_loops": 0}
    q = fast.copy(); q.precision = pkg.PRECISION_F32
    with pkg.BatchedMPC(q, B, device=0) as mpc:
        _roll(pkg, mpc, sc, 2, torch_dev, True, False, expect=-1)
        _roll(pkg, mpc, sc, 2, torch_dev, False, False, expect=-1)                   # (as the stepwise entry point refuses it)


def test_handle_state_afterwards(pkg, fast, waypoints, torch_dev):
    """A stepwise call right after a fused one on the same handle, and the reverse, cold and warm in every order: each equals the run
    of a fresh handle -- nothing of a call stays behind in the handle's warm buffer, its per-step status or its counters."""
    B, steps = 1061, 5
    sc = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=61)
    other = pkg.scenarios.lake_track_batch(B, fast, waypoints, seed=62)
    ref = {}
    for warm_start in (False, True):
        with pkg.BatchedMPC(fast, B, device=0) as mpc:
            ref[warm_start] = _roll(pkg, mpc, sc, steps, torch_dev, False, warm_start)
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        # (other cars in between: what they leave in the handle's buffers belongs to no car of `sc`)
        order = [(True, True, other), (False, True, sc), (True, True, sc), (False, False, sc), (True, False, other), (True, False, sc), (False, True, sc),
                 (True, True, other), (True, False, sc), (True, True, sc)]
        for n, (fused, warm_start, cars) in enumerate(order):
            got = _roll(pkg, mpc, cars, steps, torch_dev, fused, warm_start, want_hist=(n % 3 != 1))
            if cars is sc:
                _assert_equal(got, ref[warm_start], (n, fused, warm_start), hist=(n % 3 != 1))
        assert mpc.rollout_fused_info() == {"fused_launches": sum(1 for f, _, _ in order if f), "stepwise_loops": 0}
