"""run() and the telemetry handler on inputs no caller should send, and the adaptive fit at its edges.

What the path owes a defective instance (include/mpc_amd.h at mpc_telemetry_batch_device): a status other than SUCCESS, a launch that
ends, clean neighbours bit for bit as in a clean batch.  The CPU tests run the TEST-ONLY host build of csrc/mpc_run_core.h (mpc_twin_run)
in a child process under a time limit, so that a loop fails a test instead of hanging the suite; the gpu tests run the same batches
through the entry points and compare with the CPU build.  The fit (polyfit_qr, the order escalation) is compared with the exact answers
of tests/golden/fit_edges.json (mpmath, 120 digits; generator make_fit_edges.py), on the host build and on the device."""
import ctypes as C
import math
from fractions import Fraction
import os

import numpy as np
import pytest

import run_garbage_helpers as H
from helpers import load_golden, vp

POP_B = 64 * 3 + 37          # more than one block of the lane kernels, no multiple of the wave
FORMS = ("tel", "tel_model", "run", "run_model")
FINAL_STATUS = {0, 1, 2, 3, 4, 6}     # every MPC_STATUS_* but PENDING, which only a call with deferred tails hands out
BITWISE = ("out8", "cmd", "status", "iters", "pre", "ptsx", "ptsy", "warm")


@pytest.fixture(scope="module")
def params(pkg, golden_dir):
    return pkg.params_from_json(os.path.join(golden_dir, H.CONFIG))


@pytest.fixture(scope="module")
def pop(pkg, params, waypoints):
    return H.population(pkg, params, waypoints, POP_B)


@pytest.fixture(scope="module")
def cpu(pkg, host_twin):
    """every form, clean and dirty, cold and warm, through the CPU build -- in a child process that is killed after CHILD_TIMEOUT_S"""
    return H.run_forms_in_child(FORMS, POP_B)


@pytest.fixture(scope="module")
def fit_edges():
    return load_golden("fit_edges.json")


# ---- garbage, CPU build ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_garbage_gets_a_status_and_stays_contained_host_build(cpu, pop, form):
    """Every defect of garbage_telemetry / garbage_pose ends with a status other than SUCCESS (the well-posed entries: with a status
    code and finite numbers), cold and started warm from the clean call's records, and the clean instances behind them are bit for bit
    those of the clean batch.  With the sequential angle normalisation this test ended at the child's time limit (psi = inf, 1e300,
    1e12)."""
    names = H.names_of(form, pop)
    n = len(names)
    r = cpu[form]
    for tag, ref in (("dirty", "clean"), ("wdirty", "wclean")):
        st = r[tag]["status"]
        print("%s %s: %s" % (form, tag, ", ".join("%s -> %d" % (nm, s) for nm, s in zip(names, st[:n]))))
        assert set(np.unique(st)) <= FINAL_STATUS
        for i, nm in enumerate(names):
            if H.is_defect(nm):
                assert st[i] != 0, (form, tag, nm)
            else:
                assert np.isfinite(r[tag]["out8"][:, i]).all() and np.isfinite(r[tag]["cmd"][:, i]).all(), (form, tag, nm)
        assert (r[ref]["status"] == 0).sum() >= POP_B - 4, np.bincount(r[ref]["status"])       # the neighbours are ordinary solves
        for k in BITWISE:
            assert np.array_equal(r[tag][k][..., n:], r[ref][k][..., n:]), (form, tag, k)
    # a defective instance started warm ends as it ends cold: the record is refused or the warm attempt falls back
    assert np.array_equal(r["wdirty"]["status"][:n] != 0, r["dirty"]["status"][:n] != 0)
    assert r["wclean"]["iters"].sum() < r["clean"]["iters"].sum()                              # and the clean ones did start warm


def _sequential(a):
    """the reference's normalizeAngle (utils.h:87-92) on doubles"""
    while a >= math.pi:
        a -= 2.0 * math.pi
    while a < -math.pi:
        a += 2.0 * math.pi
    return a


def _circular(a, b):
    d = math.fmod(a - b, 2.0 * math.pi)
    return min(abs(d), abs(abs(d) - 2.0 * math.pi))


def _normalize_twin(pkg, host_twin, golden_dir, values):
    """mpc::normalize_angle through telemetry_to_pose of the host build (no latency compensation: pose[2] is the normalised psi)"""
    p = pkg.params_from_json(os.path.join(golden_dir, "config-no-latency.json"))
    assert p.latency_ms == 0
    host_twin.mpc_host_twin_tel_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    out = []
    for v in values:
        tel = np.array([1.0, 2.0, v, 30.0, 0.0, 0.1]); pose = np.zeros(6)
        host_twin.mpc_host_twin_tel_pose(C.byref(p), vp(tel), 0.0, vp(pose))
        out.append(float(pose[2]))
    return out


def test_angle_normalisation_bitwise_inside_and_exact_beyond(pkg, host_twin, golden_dir, fit_edges):
    """|psi| <= 202 (> 64 pi): bit for bit the reference's sequential subtraction.  Beyond, below 1e9: within 4 ulp(|psi|) of the exact
    remainder (mpmath, in the fixture) -- derived, not measured: psi is only known to half an ulp and the double 2 pi is off by
    3.9e-17 relative, a third of an ulp; as an angle, so across the seam at +-pi.  The oracle's restatement follows the same rule."""
    import oracle_lib as O
    rng = np.random.default_rng(3)
    inside = [0.0, -0.0, math.pi, -math.pi, np.nextafter(math.pi, 0), np.nextafter(-math.pi, -4), 64 * math.pi, -64 * math.pi, 202.0, -202.0,
              3 * math.pi, -3 * math.pi, 2 * math.pi, 1e-300] + list(rng.uniform(-7, 7, 200)) + list(rng.uniform(-202, 202, 400)) + \
             [k * math.pi for k in range(-64, 65)]
    got = _normalize_twin(pkg, host_twin, golden_dir, inside)
    for v, g in zip(inside, got):
        assert g == _sequential(v) and -math.pi <= g < math.pi, (v, g)
        assert O.lib().orc_normalize_angle(v) == g
    worst = 0.0
    beyond = fit_edges["psi"]
    got = _normalize_twin(pkg, host_twin, golden_dir, [q["psi"] for q in beyond])
    for q, g in zip(beyond, got):
        assert -math.pi <= g < math.pi, (q, g)
        assert O.lib().orc_normalize_angle(q["psi"]) == g
        if abs(q["psi"]) <= 202.0:       # the sequential region: the reference's result, which its up to 32 roundings put up to 5 ulp off
            assert g == _sequential(q["psi"])
            continue
        ratio = _circular(g, q["exact"]) / q["ulp"]
        worst = max(worst, ratio)
        assert ratio <= 4.0, (q, g, ratio)
    print("angle normalisation beyond 202 rad: worst error %.3f ulp(|psi|) of 4 allowed" % worst)
    for v in H.PSI_IN_RANGE:
        assert any(q["psi"] == v[1] for q in beyond), v          # the in-range values of garbage_telemetry are among them
    # out of range: handed on as it came (fsincos flags it); checked here on the oracle's restatement, on the host build by the child
    for v in (1e9, -1e9, 1e12, 1e300, np.inf, -np.inf):
        assert O.lib().orc_normalize_angle(v) == v
    assert math.isnan(O.lib().orc_normalize_angle(np.nan))


# ---- the fit at its edges ------------------------------------------------------------------------------------------------------------
def _groups(fit_edges, npts):
    g = {}
    for c in fit_edges["cases"]:
        if c["npts"] == npts:
            g.setdefault((c["max_fit_order"], c["max_fit_error"]), []).append(c)
    return g


def _ulp(v):
    return float(np.spacing(abs(v)))


def _residual_excess(c, x, y, exact_res):
    """the squared residual that the coefficients c leave, minus the exact minimum -- in rational arithmetic (the doubles are taken as
    the rationals they are), as the generator measures its references: what is compared is the fit, not the rounding of eight
    subtractions y - f(x), which is larger than the difference between two fits"""
    F = Fraction
    res = sum((F(float(yi)) - sum(F(float(cj)) * F(float(xi)) ** j for j, cj in enumerate(c))) ** 2 for xi, yi in zip(x, y))
    return abs(float(res - F(exact_res)))


def check_fit_group(cases, pre, px, py, what):
    """The assertions on `pre` [15, >= len(cases)] and the waypoints returned in place, for cases that went through one call.  The
    yardstick of a unique case: 8 x the larger error of numpy.linalg.lstsq and the oracle's QR against the exact answer (8 for FMA
    contraction and the summation order of the unrolled code), at least 4 ulp of the quantity.  -> worst ratio error / yardstick"""
    worst = (0.0, None)
    for i, c in enumerate(cases):
        x, y = np.array(c["x"]), np.array(c["y"])
        assert np.array_equal(px[:, i], x) and np.array_equal(py[:, i], y), (what, c["name"])      # pose (0, 0, 0): the frame change is exact
        coef = pre[6:11, i]
        nz = np.nonzero(coef)[0]
        ncoef = max(3, int(nz[-1]) + 1) if len(nz) else 3
        # (the count as `pre` shows it: the last coefficient that is not 0.  Where the fit is not unique a zero pivot may have made the
        #  highest ones 0, so only the upper end holds there; the host build's test reads the count itself)
        assert (ncoef in c["ncoef_allowed"]) if c["unique"] else (ncoef <= max(c["ncoef_allowed"])), (what, c["name"], c["max_fit_order"], ncoef, c["ncoef_allowed"])
        assert pre[4, i] == coef[0] or (np.isnan(pre[4, i]) and np.isnan(coef[0]))                   # cte0 = f(0) = c0
        if not c["unique"]:
            continue                                     # no unique answer: the count above, and the other instances of the call
        assert ncoef == c["ncoef"]
        got = {"c0": coef[0], "c1": coef[1], "epsi0": pre[5, i]}
        exact = {"c0": c["c"][0], "c1": c["c"][1], "epsi0": c["epsi0"], "res": c["res"][-1]}
        for k in exact:
            yard = max(8.0 * max(c["ref_err"]["lstsq"][k], c["ref_err"]["oracle"][k]), 4.0 * _ulp(exact[k]))
            err = abs(got[k] - exact[k]) if k != "res" else _residual_excess(coef[:ncoef], x, y, exact["res"])
            if err / yard > worst[0]:
                worst = (err / yard, "%s npts %d order %d %s: |error| %.3g, lstsq %.3g, oracle %.3g" % (
                    c["name"], c["npts"], ncoef - 1, k, err, c["ref_err"]["lstsq"][k], c["ref_err"]["oracle"][k]))
            assert err <= yard, (what, c["name"], c["npts"], ncoef, k, exact[k], err, c["ref_err"])
    return worst


def _fit_inputs(cases, ld):
    n = cases[0]["npts"]
    pose = np.zeros((6, ld)); pose[3] = 20.0
    px = np.full((n, ld), 7.25); py = np.full((n, ld), -1.5)
    for i, c in enumerate(cases):
        px[:, i] = c["x"]; py[:, i] = c["y"]
    return pose, px, py


@pytest.mark.parametrize("npts", [3, 4, 5, 6, 7, 8])
def test_fit_edges_host_build(pkg, host_twin, params, fit_edges, npts):
    worst = (0.0, None)
    total = 0
    for (mfo, mfe), cases in sorted(_groups(fit_edges, npts).items()):
        p = params.copy(); p.max_fit_order = mfo; p.max_fit_error = mfe
        B = len(cases)
        pose, px, py = _fit_inputs(cases, B)
        pre = np.zeros((15, B)); nc = np.zeros(B, dtype=np.int32)
        with np.errstate(all="ignore"):
            assert host_twin.mpc_host_twin_run_pre(C.byref(p), C.c_int64(B), C.c_int64(B), npts, vp(pose), vp(px), vp(py), vp(pre), vp(nc)) == 0
        for i, c in enumerate(cases):
            assert nc[i] in c["ncoef_allowed"], (c["name"], mfo, nc[i])
            assert (pre[6 + nc[i]:11, i] == 0).all()
        w = check_fit_group(cases, pre, px, py, "host build")
        worst = max(worst, w, key=lambda t: t[0])
        total += B
    assert total >= 35
    print("fit edges, host build, npts %d, %d cases: worst error / yardstick %.3f (%s)" % (npts, total, worst[0], worst[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [3, 4, 5, 6, 7, 8])
def test_fit_edges_device(pkg, params, fit_edges, npts):
    """mpc_run_batch_device with `pre`, ld > B: the fixture's cases of this npts, one call per setting of max_fit_order / max_fit_error
    (they are the handle's, not the instance's).  The same assertions as on the host build; the columns past B stay as they were."""
    import torch
    dev = torch.device("cuda:0")
    lib = pkg.library()
    worst = (0.0, None)
    total = 0
    with pkg.BatchedMPC(params, 64, device=0) as mpc:
        for (mfo, mfe), cases in sorted(_groups(fit_edges, npts).items()):
            p = params.copy(); p.max_fit_order = mfo; p.max_fit_error = mfe
            mpc.set_params(p)
            B = len(cases); ld = B + 5
            assert B <= 64
            pose, px, py = _fit_inputs(cases, ld)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            d_pose, d_px, d_py = t(pose), t(px), t(py)
            d_out8 = torch.full((8, ld), -3.0, dtype=torch.float64, device=dev); d_pre = torch.full((15, ld), -3.0, dtype=torch.float64, device=dev)
            d_st = torch.full((ld,), -3, dtype=torch.int32, device=dev); d_it = torch.full((ld,), -3, dtype=torch.int32, device=dev)
            q = lambda x: C.c_void_p(x.data_ptr())
            rc = lib.mpc_run_batch_device(mpc._h, C.c_int64(B), C.c_int64(ld), C.c_int(npts), q(d_pose), q(d_px), q(d_py), q(d_out8), None, q(d_st),
                                          q(d_it), q(d_pre), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert rc == 0, lib.mpc_last_error()
            torch.cuda.synchronize()
            g_pre, g_px, g_py, g_st = d_pre.cpu().numpy(), d_px.cpu().numpy(), d_py.cpu().numpy(), d_st.cpu().numpy()
            assert np.array_equal(g_px[:, B:], px[:, B:]) and np.array_equal(g_py[:, B:], py[:, B:])      # past B: untouched
            assert (g_pre[:, B:] == -3.0).all() and (g_st[B:] == -3).all() and (d_out8.cpu().numpy()[:, B:] == -3.0).all()
            assert set(np.unique(g_st[:B])) <= FINAL_STATUS
            w = check_fit_group(cases, g_pre, g_px, g_py, "device")
            worst = max(worst, w, key=lambda t_: t_[0])
            total += B
    assert total >= 35
    print("fit edges, device, npts %d, %d cases: worst error / yardstick %.3f (%s)" % (npts, total, worst[0], worst[1]))


# ---- garbage, device ------------------------------------------------------------------------------------------------------------
def _device_run(pkg, mpc, form, x, px, py, model, warm=None, warm_status=None, want_warm=False):
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None
    tel = form.startswith("tel")
    kw = dict(model=t(model), want_warm=want_warm)
    if warm is not None:
        kw.update(warm=t(warm), warm_status=t(np.ascontiguousarray(warm_status, dtype=np.int32)))
    d_px, d_py = t(px), t(py)
    if tel:
        r = mpc.telemetry_torch(t(x), d_px, d_py, extra_latency=H.EXTRA_LATENCY, want_out8=True, **kw)
    else:
        r = mpc.run_torch(t(x), d_px, d_py, want_pre=True, **kw)
    torch.cuda.synchronize()
    st = mpc.stats()
    out = {k: v.cpu().numpy() for k, v in r.items() if v is not None}
    out["ptsx"], out["ptsy"] = d_px.cpu().numpy(), d_py.cpu().numpy()
    counts = st.n_success + st.n_maxiter + st.n_linesearch + st.n_infeasible + st.n_numeric + st.n_acceptable + st.n_pending
    assert st.batch == x.shape[1] and counts == x.shape[1], (st.batch, counts)
    assert st.n_success == int((out["status"] == 0).sum())
    return out


def _dirty_and_clean(form, pop, B):
    tel = form.startswith("tel")
    model = pop["model"][:, :B] if form.endswith("_model") else None
    x = (pop["tel"] if tel else pop["pose"])[:, :B]
    px, py = pop["ptsx"][:, :B], pop["ptsy"][:, :B]
    gx, gpx, gpy, gm, names = (H.garbage_telemetry if tel else H.garbage_pose)(x, px, py, model)
    return (x, px, py, model), (gx, gpx, gpy, gm), names


def _assert_device_follows_cpu(form, names, clean, dirty, cpu_dirty, what, keys=("out8", "cmd", "status", "iters")):
    n = len(names)
    same = H.same_status(dirty["status"][:n], cpu_dirty["status"][:n])
    print("%s: %s" % (what, ", ".join("%s -> %d" % (nm, s) for nm, s in zip(names, dirty["status"][:n]))))
    assert same.all(), (what, [(nm, int(a), int(b)) for nm, a, b in zip(names, dirty["status"][:n], cpu_dirty["status"][:n])])
    for k in keys:
        if k in dirty and k in clean:
            assert np.array_equal(dirty[k][..., n:], clean[k][..., n:]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("form,B,wave_max_batch", [("tel", POP_B, 0), ("run", POP_B, 0), ("tel", POP_B, -1), ("run", POP_B, -1),
                                                   ("tel", 48, 0), ("run", 48, 0), ("tel", 48, -1), ("run", 48, -1),
                                                   ("tel_model", POP_B, 0), ("run_model", 48, -1)])
def test_garbage_gets_a_status_and_stays_contained_device(pkg, params, pop, cpu, form, B, wave_max_batch):
    """mpc_telemetry_batch_device / mpc_run_batch_device (and their _model forms) on the batches the CPU build has been through
    (fixture `cpu`: this test runs on a tree on which that one passes): B = 229 and 48, the wave kernels and, with wave_max_batch = -1,
    the lane kernel.  The statuses of the CPU build (2 and 4 interchangeable), the clean neighbours bit for bit, and mpc_get_stats adds up."""
    p = params.copy(); p.wave_max_batch = wave_max_batch
    cl, di, names = _dirty_and_clean(form, pop, B)
    n = len(names)
    with pkg.BatchedMPC(p, B, device=0) as mpc:
        clean = _device_run(pkg, mpc, form, *cl)
        dirty = _device_run(pkg, mpc, form, *di)
    _assert_device_follows_cpu(form, names, clean, dirty, cpu[form]["dirty"], "%s B=%d wave_max_batch=%d" % (form, B, wave_max_batch),
                               keys=("out8", "cmd", "status", "iters", "ptsx", "ptsy", "pre"))
    for i, nm in enumerate(names):
        if H.is_defect(nm):
            assert dirty["status"][i] != 0, nm


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["tel", "run"])
def test_garbage_started_warm_falls_back_device(pkg, params, pop, cpu, form):
    """The _warm forms: a clean call writes the records, then the dirty batch starts warm from them.  The defective instances end as
    they end cold (the status of the CPU build), the clean ones are bit for bit the clean warm batch."""
    B = POP_B
    cl, di, names = _dirty_and_clean(form, pop, B)
    n = len(names)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        first = _device_run(pkg, mpc, form, *cl, want_warm=True)
        wclean = _device_run(pkg, mpc, form, *cl, warm=first["warm"], warm_status=first["status"])
        wdirty = _device_run(pkg, mpc, form, *di, warm=first["warm"], warm_status=first["status"])
    if "iters" in first:
        assert wclean["iters"][n:].sum() < first["iters"][n:].sum()
    _assert_device_follows_cpu(form, names, wclean, wdirty, cpu[form]["wdirty"], "%s warm" % form, keys=("out8", "cmd", "status", "iters", "warm"))
    for i, nm in enumerate(names):
        if H.is_defect(nm):
            assert wdirty["status"][i] != 0, nm


@pytest.mark.gpu
def test_garbage_through_the_host_entry_points(pkg, params, pop, cpu):
    """mpc_telemetry_batch_host and mpc_wire_telemetry_batch_host (the structs a parser would have filled, had it let them through)."""
    B = 48
    cl, di, names = _dirty_and_clean("tel", pop, B)
    n = len(names)
    lib = pkg.library()
    p = lambda a: C.c_void_p(a.ctypes.data)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)

    def host(x, px, py):
        cmd = np.zeros((2, B)); st = np.zeros(B, dtype=np.int32)
        x, px, py = f(x), f(px), f(py)
        assert lib.mpc_telemetry_batch_host(mpc._h, C.c_int64(B), C.c_int64(B), C.c_int(px.shape[0]), p(x), C.c_double(H.EXTRA_LATENCY), p(px), p(py), p(cmd), p(st)) == 0
        return {"cmd": cmd, "status": st}

    def wire(x, px, py):
        W = (pkg.MpcWireTelemetry * B)()
        for i in range(B):
            W[i].x, W[i].y, W[i].psi, W[i].speed, W[i].steering_angle = (float(v) for v in x[:5, i])
            W[i].npts = px.shape[0]
            for k in range(px.shape[0]):
                W[i].ptsx[k] = float(px[k, i]); W[i].ptsy[k] = float(py[k, i])
        prev = f(x[5])
        cmd = np.zeros((2, B)); st = np.zeros(B, dtype=np.int32)
        assert lib.mpc_wire_telemetry_batch_host(mpc._h, C.c_int64(B), W, p(prev), C.c_double(H.EXTRA_LATENCY), p(cmd), p(st)) == 0
        return {"cmd": cmd, "status": st}

    with pkg.BatchedMPC(params, B, device=0) as mpc:
        for name, fn in (("mpc_telemetry_batch_host", host), ("mpc_wire_telemetry_batch_host", wire)):
            clean, dirty = fn(*cl[:3]), fn(*di[:3])
            _assert_device_follows_cpu("tel", names, clean, dirty, cpu["tel"]["dirty"], name, keys=("cmd", "status"))
            assert all(dirty["status"][i] != 0 for i, nm in enumerate(names) if H.is_defect(nm))
