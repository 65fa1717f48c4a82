"""The fused rollout (mpc_rollout_batch_device_fused) checked without a GPU: the rule one car follows between two of its solves
(mpc::RolloutCar, csrc/mpc_core.h), run car by car by the CPU build tests/host_twin (mpc_twin_rollout), against the step-by-step closed loops of
tests/host_twin (mpc_twin_solve); and the two symbols of the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rollout_fused_helpers import load_rollout_twin, twin_rollout
from warm_helpers import load_warm_twin, twin_closed_loop

CARS, STEPS = 96, 25


@pytest.fixture(scope="module")
def twins():
    return load_rollout_twin(), load_warm_twin()


@pytest.fixture(scope="module")
def cars(pkg, golden_dir, waypoints):
    params = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    return params, pkg.scenarios.lake_track_batch(CARS, params, waypoints, seed=122)


@pytest.mark.parametrize("mode", ["cold", "warm", "warm_shift1"])
def test_car_by_car_is_step_by_step_bitwise(pkg, twins, cars, mode):
    """96 cars x 25 steps: every solve of the car-by-car loop -- its 9-vector, status and iterations -- is bitwise the solve of the
    step-by-step loop, and what the call reports per car is the fold of its steps."""
    roll, warm_twin = twins
    params, sc = cars
    opts = pkg.warm_opts_default(shift=1) if mode == "warm_shift1" else pkg.warm_opts_default()
    warm_start = mode != "cold"
    hist, sst, sit = twin_closed_loop(warm_twin, params, sc, STEPS, opts, warm_start=warm_start)
    r = twin_rollout(roll, params, sc, STEPS, opts, warm_start)
    assert np.array_equal(r["hist"], hist, equal_nan=True)
    assert np.array_equal(r["step_status"], sst) and np.array_equal(r["step_iters"], sit)
    assert np.array_equal(r["state"], hist[-1, :6], equal_nan=True)
    assert np.array_equal(r["status"], sst.max(0)) and np.array_equal(r["iters"], sit.sum(0))


def test_fused_abi(pkg):
    """The two symbols exist with the signatures of include/mpc_amd.h; the info call refuses NULL."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    header = open(os.path.join(_abi.ROOT, "include", "mpc_amd.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int mpc_rollout_batch_device_fused(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs, "
            "const double *yaw_lo, const double *yaw_hi, const double *weights, int warm_start, const MpcWarmOpts *opts, double *hist, "
            "int32_t *status, int32_t *iters, void *stream);") in flat
    assert "int mpc_rollout_fused_info(const MpcHandle *h, int64_t *out2);" in flat
    assert hasattr(lib, "mpc_rollout_batch_device_fused") and hasattr(lib, "mpc_rollout_fused_info")
    DP = C.c_void_p
    assert lib.mpc_rollout_batch_device_fused.argtypes == ([C.c_void_p, C.c_int64, C.c_int64, C.c_int] + [DP] * 5 +
                                                            [C.c_int, C.POINTER(pkg.MpcWarmOpts)] + [DP] * 3 + [C.c_void_p])
    assert lib.mpc_rollout_fused_info.argtypes == [C.c_void_p, C.POINTER(C.c_int64)]
    out2 = (C.c_int64 * 2)(7, 7)
    assert lib.mpc_rollout_fused_info(None, out2) == -1 and list(out2) == [7, 7]
    # a NULL handle is refused before anything is touched, cold and warm, as the stepwise entry points refuse it
    assert lib.mpc_rollout_batch_device_fused(None, 64, 64, 2, None, None, None, None, None, 0, None, None, None, None, None) == -1
    assert lib.mpc_rollout_batch_device_fused(None, 64, 64, 2, None, None, None, None, None, 1, None, None, None, None, None) == -1
    assert lib.mpc_abi_version() == 5
