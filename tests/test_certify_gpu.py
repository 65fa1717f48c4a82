"""The certificate of a stored point on the device (mpc_certify_batch_device / _host, include/mpc_amd_certify.h): mpc_certify_kernel
against the CPU build of the same function bit for bit, against the oracle's derivatives on the device's own records, the verdict
against the status of the solve that wrote them, the run() path, the host form, the handles that are served and refused, and the
containment of bad instances.  Every output array holds sentinels before a call, every input not-a-number from column B on."""
import numpy as np
import pytest

import certify_helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def twin():
    return H.load_certify_twin()


def _with(params, **kw):
    p = params.copy()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _shape(pkg, golden_dir, waypoints, N, B, dt=None, mixed=False):
    """-> (cfgname, overrides, params (no fp32 start: the plain warm call is refused on such a handle), batch, the optional arrays)"""
    if mixed:
        cfgname, over, params, b, weights, model, horizon = H.mixed_batch(pkg, golden_dir, waypoints, B)
        return cfgname, over, params, b, dict(weights=weights, model=model, horizon=horizon)
    cfgname, over, params, b = H.plain_batch(pkg, golden_dir, waypoints, N, B, dt=dt)
    return cfgname, over, _with(params, f64_f32_start=0), b, {}


@pytest.fixture(scope="module")
def b65(pkg, golden_dir, waypoints, dev):
    """N = 10, B = 65 with the records of the device's cold warm-capable solve (shared, read-only)"""
    cfgname, over, params, b, kw = _shape(pkg, golden_dir, waypoints, 10, 65)
    with pkg.BatchedMPC(params, 65, device=0) as mpc:
        res = H.device_records(pkg, mpc, dev, b)
    return cfgname, over, params, b, res


@pytest.fixture(scope="module")
def mixed130(pkg, golden_dir, waypoints, dev):
    cfgname, over, params, b, kw = _shape(pkg, golden_dir, waypoints, 10, 130, mixed=True)
    with pkg.BatchedMPC(params, 130, device=0) as mpc:
        res = H.device_records(pkg, mpc, dev, b, **kw)
    return cfgname, over, params, b, kw, res


def test_symbols_are_there_before_anything_else(pkg):
    lib = pkg.library()
    assert hasattr(lib, "mpc_certify_batch_device") and hasattr(lib, "mpc_certify_batch_host")


@pytest.mark.parametrize("N,dt,B,ld,ld_sol,mixed", [(10, None, 1, None, None, False), (10, None, 65, 96, 80, False), (10, None, 300, None, None, False),
                                                    (3, None, 65, None, None, False), (25, 0.05, 70, None, None, False), (10, None, 130, None, None, True)])
def test_device_equals_cpu_build_bitwise(pkg, golden_dir, waypoints, dev, twin, N, dt, B, ld, ld_sol, mixed):
    cfgname, over, params, b, kw = _shape(pkg, golden_dir, waypoints, N, B, dt=dt, mixed=mixed)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        res = H.device_records(pkg, mpc, dev, b, **kw)
        got = H.device_certify(pkg, mpc, dev, b, res["warm"], ld=ld, ld_sol=ld_sol, **kw)
    assert got["rc"] == 0, got["msg"]
    ref = H.twin_certify(twin, params, b, res["warm"], **kw)
    H.assert_same_bits(got, ref, B, what=(N, B))
    assert (got["cert"][:, B:] == H.SENTINEL).all() and (got["verdict"][B:] == H.ISENTINEL).all()
    assert np.isin(got["verdict"][:B], (H.CONVERGED, H.CERT_ACCEPTABLE, H.NOT_CONVERGED, H.NOT_A_POINT, H.NO_PROBLEM)).all()


def test_oracle_parity_on_the_devices_own_records(pkg, dev, b65):
    cfgname, over, params, b, res = b65
    with pkg.BatchedMPC(params, 65, device=0) as mpc:
        def certify(s):
            r = H.device_certify(pkg, mpc, dev, b, s)
            assert r["rc"] == 0, r["msg"]
            return r
        H.assert_parity(pkg, certify, cfgname, over, params, b, res["warm"], res["status"], what="device B=65")


def test_oracle_parity_on_the_mixed_batch(pkg, dev, mixed130):
    cfgname, over, params, b, kw, res = mixed130
    with pkg.BatchedMPC(params, 130, device=0) as mpc:
        def certify(s):
            r = H.device_certify(pkg, mpc, dev, b, s, **kw)
            assert r["rc"] == 0, r["msg"]
            return r
        H.assert_parity(pkg, certify, cfgname, over, params, b, res["warm"], res["status"], what="device mixed", **kw)
        got = certify(res["warm"])
    ok = res["status"] != 3
    assert np.all(np.abs(got["cert"][H.OBJ, ok] - res["out"][8, ok]) <= 1e-12 * np.abs(res["out"][8, ok]))
    H.assert_verdicts(params, b, res, got, model=kw["model"], what="device mixed")


def test_verdict_against_status(pkg, golden_dir, waypoints, dev):
    cfgname, over, params, b, kw = _shape(pkg, golden_dir, waypoints, 10, 300)
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with pkg.BatchedMPC(params, 300, device=0) as mpc:
        res = H.device_records(pkg, mpc, dev, b)
        r = mpc.certify_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), t(res["warm"]))        # (the Python binding)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in r.items()}
        raw = H.device_certify(pkg, mpc, dev, b, res["warm"])
    H.assert_same_bits(got, raw, 300, what="certify_torch")
    ok = res["status"] != 3
    assert np.all(np.abs(got["cert"][H.OBJ, ok] - res["out"][8, ok]) <= 1e-12 * np.abs(res["out"][8, ok]))
    H.assert_verdicts(params, b, res, got, what="device B=300", min_success=250)


def test_run_path_is_certified_from_pre_and_warm_out(pkg, golden_dir, waypoints, dev):
    """mpc_run_batch_device_warm with warm_in = NULL writes warm_out and pre [15][ld]: rows 0-5 the state, 6-10 the coefficients, 11 and
    12 the psi bounds, passed with the same ld."""
    import os
    import torch
    B = 33
    params = _with(pkg.params_from_json(os.path.join(golden_dir, "config-fast.json")), f64_f32_start=0)
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=31)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    with pkg.BatchedMPC(params, B, device=0) as mpc:
        r = mpc.run_torch(t(sc["pose"]), t(sc["ptsx"]), t(sc["ptsy"]), want_pre=True, want_warm=True)
        pre = r["pre"]
        c = mpc.certify_torch(pre[0:6], pre[6:11], pre[11], pre[12], r["warm"])
        torch.cuda.synchronize()
    status, verdict, cert = r["status"].cpu().numpy(), c["verdict"].cpu().numpy(), c["cert"].cpu().numpy()
    assert (status == 0).sum() >= 25, np.bincount(status)
    assert (verdict[status == 0] == H.CONVERGED).all(), (status, verdict)
    assert (cert[H.NLP_ERROR, status == 0] <= params.tol).all() and np.isin(verdict[status == 6], (H.CONVERGED, H.CERT_ACCEPTABLE)).all()


def test_host_form_and_handles(pkg, dev, b65):
    cfgname, over, params, b, res = b65
    with pkg.BatchedMPC(params, 65, device=0) as mpc:
        d = H.device_certify(pkg, mpc, dev, b, res["warm"])
        h = H.device_certify(pkg, mpc, dev, b, res["warm"], host=True, ld=70, ld_sol=66)
        n = mpc.certify_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], res["warm"])
        refusals = [H.device_certify(pkg, mpc, dev, b, res["warm"], ld=64), H.device_certify(pkg, mpc, dev, b, res["warm"], ld_sol=64),
                    H.device_certify(pkg, mpc, dev, b, res["warm"], host=True, ld_sol=64)]
    assert d["rc"] == 0 and h["rc"] == 0, (d["msg"], h["msg"])
    H.assert_same_bits(h, d, 65, what="host form")
    H.assert_same_bits(n, d, 65, what="certify_numpy")
    assert (h["cert"][:, 65:] == H.SENTINEL).all() and (h["verdict"][65:] == H.ISENTINEL).all()
    assert [r["rc"] for r in refusals] == [-1, -1, -1] and "ld_sol < B" in refusals[1]["msg"], refusals
    with pkg.BatchedMPC(params, 64, device=0) as small:
        r = H.device_certify(pkg, small, dev, b, res["warm"])
        assert r["rc"] == -1 and (r["cert"] == H.SENTINEL).all(), r["msg"]          # B above the handle's capacity
    with pkg.BatchedMPC(_with(params, f64_f32_start=1), 65, device=0) as started32:
        s = H.device_certify(pkg, started32, dev, b, res["warm"])
    assert s["rc"] == 0, s["msg"]
    H.assert_same_bits(s, d, 65, what="f64_f32_start = 1")
    with pkg.BatchedMPC(_with(params, precision=1), 65, device=0) as f32:
        for host in (False, True):
            r = H.device_certify(pkg, f32, dev, b, res["warm"], host=host)
            assert r["rc"] == -1 and "MPC_PRECISION_F32" in r["msg"] and (r["cert"] == H.SENTINEL).all(), r


def test_containment_on_the_device(pkg, dev, twin, b65):
    cfgname, over, params, b, res = b65
    clean, dirty = H.containment_case(pkg, params, b, res["warm"])
    with pkg.BatchedMPC(params, 65, device=0) as mpc:
        run = lambda k: H.device_certify(pkg, mpc, dev, k["batch"], k["sol"], model=k["model"], horizon=k["horizon"])
        c, d = run(clean), run(dirty)
    assert c["rc"] == 0 and d["rc"] == 0
    H.assert_contained(c, d, params)
    H.assert_same_bits(d, H.twin_certify(twin, params, dirty["batch"], dirty["sol"], model=dirty["model"], horizon=dirty["horizon"]), 65, what="dirty")
