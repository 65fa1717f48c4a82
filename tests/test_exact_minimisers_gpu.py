"""Every device solve path against the EXACT minimisers of tests/golden/exact_minimisers.npz (see tests/test_exact_minimisers.py and
tests/golden/make_exact_minimisers.py): one assertion for all of them -- exact_helpers.assert_exact: every case SUCCESS, every quantity
within the class yardstick (8 x the oracle's own distance to the exact value) -- and the certificate kernels at stored exact
primal-dual points.  Every test is one or two launches per handle of at most 37 instances.

Run as a script it prints the measured maxima as JSON (profiles/exact_minimisers.json):
    python tests/test_exact_minimisers_gpu.py --device        the device paths below
    python tests/test_exact_minimisers_gpu.py                 the CPU twin's paths (exact_helpers.twin_paths)"""
import json
import os
import sys

import numpy as np
import pytest

from exact_helpers import MEASURED, assert_certificates, assert_exact, fixture, group_params, record_groups, reorder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _device_solve(pkg, params, g, dev, warm=None, warm_status=None, want_warm=False, model=True, warm_opts=None):
    """one launch of the entry point the arguments name on a handle of `params` -> numpy"""
    import torch
    t = lambda a, dt=np.float64: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    b = g["batch"]
    with pkg.BatchedMPC(params, len(g["idx"]), device=0) as mpc:
        r = mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), weights=t(g["weights"]), want_traj=True,
                            model=t(g["model"]) if model else None, horizon=t(g["horizon"], np.int32), warm=t(warm), warm_status=t(warm_status, np.int32),
                            want_warm=want_warm, warm_opts=warm_opts)
        torch.cuda.synchronize()
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}


def _host_solve(pkg, params, g):
    b = g["batch"]
    with pkg.BatchedMPC(params, len(g["idx"]), device=0) as mpc:
        return mpc.solve_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], weights=g["weights"], want_traj=True)


def _plain(pkg, dev, classes, path, host=False, **over):
    for cls in classes:
        for g in fixture().groups(cls):
            p = group_params(pkg, g, **over)
            assert_exact(g, _host_solve(pkg, p, g) if host else _device_solve(pkg, p, g, dev), path)


def _warm(pkg, dev, cls, path):
    opts = pkg.warm_opts_default(shift=0)
    for g in fixture().groups(cls):
        p = group_params(pkg, g, f64_f32_start=0)
        cold = _device_solve(pkg, p, g, dev, want_warm=True, warm_opts=opts)
        assert_exact(g, cold, path + ", cold")
        again = _device_solve(pkg, p, g, dev, warm=cold["warm"], warm_status=cold["status"], warm_opts=opts)
        assert_exact(g, again, path + ", warm")


# path name -> function(pkg, dev): what `--device` runs and what the tests below call, one each
DEVICE_PATHS = {
    "device wave kernels": lambda pkg, dev: _plain(pkg, dev, ("plain", "a_free"), "device wave kernels"),
    "device lane kernel": lambda pkg, dev: _plain(pkg, dev, ("plain", "a_free"), "device lane kernel", wave_max_batch=-1),
    "device horizons": lambda pkg, dev: _plain(pkg, dev, ("horizons",), "device horizons", f64_f32_start=0),
    "device weights": lambda pkg, dev: _plain(pkg, dev, ("weights",), "device weights"),
    "device host form": lambda pkg, dev: _plain(pkg, dev, ("plain",), "device host form", host=True),
    "device max_soc 4": lambda pkg, dev: _plain(pkg, dev, ("plain",), "device max_soc 4", max_soc=4),
    "device initial_state_rows": lambda pkg, dev: _plain(pkg, dev, ("plain",), "device initial_state_rows", initial_state_rows=1),
    "device _warm": lambda pkg, dev: _warm(pkg, dev, "plain", "device _warm"),
    "device _warm_model": lambda pkg, dev: _warm(pkg, dev, "model", "device _warm_model"),
}


def _f32_start(pkg, dev):
    for g in fixture().groups("horizons", N=25):
        assert_exact(g, _device_solve(pkg, group_params(pkg, g, f64_f32_start=1), g, dev), "device f64_f32_start")


def _model(pkg, dev):
    for g in fixture().groups("model"):
        assert_exact(g, _device_solve(pkg, group_params(pkg, g), g, dev), "device _model")


def _mixed(pkg, dev):
    for g in fixture().groups("mixed_horizon"):
        for tag, gg in (("fixture order", g), ("sorted", reorder(g, np.argsort(g["horizon"], kind="stable")))):
            assert_exact(gg, _device_solve(pkg, group_params(pkg, gg), gg, dev), "device _horizon, " + tag)


DEVICE_PATHS.update({"device f64_f32_start": _f32_start, "device _model": _model, "device _horizon": _mixed})


@pytest.mark.parametrize("path", sorted(DEVICE_PATHS))
def test_device_path(pkg, torch_dev, path):
    """mpc_solve_batch_device (the default handle: the wave kernels at these sizes; wave_max_batch = -1: the lane kernel with a partial
    last wavefront; handles of N = 3, 4, 17, 25, N = 25 also with f64_f32_start on; per-instance weights; max_soc = 4;
    initial_state_rows = 1), mpc_solve_batch_host, _model, _horizon in the fixture's order and sorted by horizon, and _warm /
    _warm_model cold and then warm from their own warm_out: each held to the exact minimisers, every case of every class it serves."""
    DEVICE_PATHS[path](pkg, torch_dev)
    assert any(p.startswith(path) for p in MEASURED)


@pytest.mark.parametrize("host", (False, True), ids=("device", "host"))
def test_certificates_at_exact_points(pkg, torch_dev, host):
    """mpc_certify_batch_device and mpc_certify_batch_host at the 24 exact primal-dual points and their perturbed copies: the rows
    against the generator's 70-digit values within the rounding bounds of certify_helpers.assert_rows, and the verdict the header's
    rule gives on those rows (tests/test_exact_minimisers.py::test_certify_twin_at_exact_points says which and why)."""
    from certify_helpers import device_certify
    for g in record_groups():
        with pkg.BatchedMPC(group_params(pkg, g), len(g["idx"]), device=0) as mpc:
            def certify(sol):
                r = device_certify(pkg, mpc, torch_dev, g["batch"], sol, weights=g["weights"], model=g["model"], horizon=g["horizon"], host=host)
                assert r["rc"] == 0, r["msg"]
                return r
            assert_certificates(g, certify, "certify host" if host else "certify device")


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as G
    pkg = G.load_package()
    if "--device" in argv:
        import torch
        dev = torch.device("cuda:0")
        for name in sorted(DEVICE_PATHS):
            DEVICE_PATHS[name](pkg, dev)
        what = "device"
    else:
        from exact_helpers import twin_paths
        for name, run in sorted(twin_paths(pkg).items()):
            run()
        what = "twin"
    fx = fixture()
    print(json.dumps({"what": what, "fixture": "tests/golden/exact_minimisers.npz", "cases": fx.n, "classes": {c: int(len(fx.of_class(c))) for c in fx.classes},
                      "quantities": "steer [rad], accel [m/s^2], state (step-1), traj [m]: max |got - exact|; cost: relative",
                      "yardsticks": fx.yard, "measured": MEASURED}, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
