"""The track drive under noise without a GPU (include/mpc_amd_noise.h): the generator's known answers, the one draw function against an
independent numpy statement of it and against the statistics a normal stream must have, the CPU build of the noisy drive
(tests/drive_twin/noise_drive_twin.cpp) -- what it equals with no noise, that nothing depends on a car's index, the sensing, acting and
dropping rules to the last bit, the columns that cannot be used --, the ABI's host-only functions and declarations, the Python layer's
argument checks, and the CPU build under AddressSanitizer + UndefinedBehaviorSanitizer as a program of its own."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import budget_helpers as BH
import drive_helpers as D
import drive_latency_helpers as DL
import drive_plant_helpers as DP
import noise_helpers as NH
from drive_horizon_helpers import mixed_horizons
from helpers import ROOT
from model_helpers import draw_rows
from noise_helpers import DROP, POS, PSI, SEED, SPEED, STEER, DRIFT, same, twin_noise_drive

B7, STEPS = 7, 4


@pytest.fixture(scope="module")
def twin():
    return NH.load_noise_drive_twin()


@pytest.fixture(scope="module")
def pop(pkg, golden_dir, waypoints):
    """config-fast.json at N = 10 and 7 cars on the lake track"""
    params = BH.fast_params(pkg, golden_dir)
    return params, pkg.scenarios.track_starts(B7, params, waypoints, seed=6)


@pytest.fixture(scope="module")
def draws(pkg):
    """the stated (seed, step) pairs: mpc_drive_noise_draw and the numpy statement, computed once, never changed"""
    seed, step = NH.stated_pairs()
    ref, rad = NH.np_draw(seed.astype(np.uint64), step)
    return {"seed": seed, "step": step, "lib": NH.lib_draws(pkg.library(), seed, step), "ref": ref, "rad": rad}


def _opts(pkg, params, warm):
    return pkg.drive_opts_default(params, warm_start=warm), pkg.warm_opts_default()


def test_philox_known_answers(pkg):
    """Philox4x32-10's known answers (Random123's kat_vectors: counter and key all zero, all ones, and the digits of pi) through
    mpc_debug_philox4x32, and the numpy generator of noise_helpers on the same three."""
    lib = pkg.library()
    kat = (([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        c, k, o = np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
        assert lib.mpc_debug_philox4x32(c.ctypes.data, k.ctypes.data, o.ctypes.data) == 0
        assert " ".join("%08x" % v for v in o) == want
        assert " ".join("%08x" % int(v) for v in NH.np_philox4x32([[x] for x in ctr], [[x] for x in key])[:, 0]) == want
    assert lib.mpc_debug_philox4x32(None, k.ctypes.data, o.ctypes.data) == -1


def test_draw_against_numpy(pkg, twin, draws):
    """mpc_drive_noise_draw on seeds 1000 .. 1255 x steps 0 .. 255 and on seeds 0, 2^32 - 1, 2^32, 2^53 - 1 at steps 0 and 2^31 - 1
    against noise_helpers.np_draw: u_drop bitwise -- it is (r + 0.5) * 2^-32, exact --, each normal within rad * NH.DRAW_REL.

    The bound, derived at noise_helpers.DRAW_REL: z = rad * t with rad = sqrt(-2 ln u_a), t the cosine or sine of
    theta = fl(6.283185307179586 * u_b), the same double on both sides.  The library's t is within 4e-16 absolute of the exact one and
    its logarithm within 2.3e-16 relative (the bounds tests/test_math_conformance.py holds fp64 fsincos and flog to), so its rad is
    within 2.3e-16 / 2 relative plus half an ulp of the square root, and the product adds half an ulp.  numpy's log, cos and sin are
    given one ulp each (2^-53 relative on rad, 2^-52 absolute on t) and the same two half ulps.  With |t| <= 1 that is
    rad * (4e-16 + 2.3e-16 / 2 + 7 * 2^-53), and one more 2^-53 for the products of two errors: 1.40e-15 * rad.
    The CPU build of the test library draws the library's bits."""
    lib, ref, rad = draws["lib"], draws["ref"], draws["rad"]
    assert np.isfinite(lib).all() and np.array_equal(lib[6], ref[6]) and (lib[6] > 0).all() and (lib[6] < 1).all()
    assert abs(NH.DRAW_REL - (4e-16 + 2.3e-16 / 2 + 8 * 2.0 ** -53)) < 1e-30
    err = np.abs(lib[:6] - ref[:6])
    print("draws: max |z - z_numpy| / (rad * DRAW_REL) = %.3f, max |z| = %.2f" % ((err / (rad[:6] * NH.DRAW_REL)).max(), np.abs(ref[:6]).max()))
    assert (err <= rad[:6] * NH.DRAW_REL).all()
    sub = np.r_[0:65536:97, 65536:65544]
    assert np.array_equal(NH.lib_draws(twin, draws["seed"][sub], draws["step"][sub], "mpc_noise_drive_twin_draw"), lib[:, sub])


def test_draw_statistics(draws):
    """The 65 536 draws of the grid, per channel: |mean| <= 4 / sqrt(n), |var - 1| <= 4 sqrt(2 / n), every cross-channel correlation
    and the lag-1 products over steps and over seeds <= 4 / sqrt(n); the share of u_drop < 0.25 within 4 sqrt(0.25 * 0.75 / n) of 0.25."""
    n = 65536
    z, u = draws["lib"][:6, :n], draws["lib"][6, :n]
    lim = 4 / np.sqrt(n)
    mean, var = z.mean(1), z.var(1)
    print("max |mean| %.4f (bound %.4f), max |var - 1| %.4f (bound %.4f)" % (np.abs(mean).max(), lim, np.abs(var - 1).max(), 4 * np.sqrt(2 / n)))
    assert (np.abs(mean) <= lim).all() and (np.abs(var - 1) <= 4 * np.sqrt(2 / n)).all()
    cc = (z @ z.T) / n
    off = np.abs(cc - np.diag(np.diag(cc)))
    grid = z.reshape(6, 256, 256)                 # [channel, seed, step]
    lag_step = (grid[:, :, 1:] * grid[:, :, :-1]).mean((1, 2))
    lag_seed = (grid[:, 1:, :] * grid[:, :-1, :]).mean((1, 2))
    print("max |cross| %.4f, max |lag-1 over steps| %.4f, over seeds %.4f (bound %.4f)" % (off.max(), np.abs(lag_step).max(), np.abs(lag_seed).max(), lim))
    assert (off <= lim).all() and (np.abs(lag_step) <= lim).all() and (np.abs(lag_seed) <= lim).all()
    share = (u < 0.25).mean()
    assert abs(share - 0.25) <= 4 * np.sqrt(0.25 * 0.75 / n), share


def test_null_noise_is_the_budget_twin_and_the_zero_column_is_null(pkg, twin, pop, waypoints):
    """noise = NULL (seen NULL or given) is libbudget_drive_twin's bits, plain and with every other column, cold and warm; seen then
    holds the true cars; the zero column (any seed) is noise = NULL."""
    params, car = pop
    bt = BH.load_budget_drive_twin()
    model, lat, plant, hz = draw_rows(params, B7, seed=9), DL.draw_latency(B7), DP.draw_plant(B7), mixed_horizons(B7)
    budget = np.array([3, 50, 8, 50, 4, 50, 50], dtype=np.int32)
    for warm in (0, 1):
        o, wo = _opts(pkg, params, warm)
        for kw in ({}, dict(model=model, horizon=hz, latency=lat, plant=plant, budget=budget)):
            want = BH.twin_budget_drive(bt, params, waypoints, car, STEPS, o, wo, **kw)
            for seen in (False, True):
                got = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, None, seen=seen, pad=3, **kw)
                same(got, want, keys=("car", "summary", "hist", "status", "iters", "handler_status"), what="noise = NULL")
            assert np.array_equal(got["seen"], got["hist"][:, 0:4])
            zero = NH.noise_columns(B7, {})
            same(twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, zero, pad=3, **kw), got, what="the zero column")
            assert np.array_equal(pkg.drive_noise_default(B7, zero[SEED].astype(np.int64)), zero)


def test_nothing_depends_on_the_index(pkg, twin, pop, waypoints):
    """Permuting the cars (seeds with them) permutes every output bitwise; two cars with the same start and seed are equal, and with
    different seeds differ."""
    params, car = pop
    nz = NH.noise_columns(B7)
    perm = np.array([3, 0, 6, 1, 5, 2, 4])
    twins = car.copy(); twins[:, 1] = car[:, 0]; twins[:, 2] = car[:, 0]
    nz2 = nz.copy(); nz2[SEED, 1] = nz[SEED, 0]
    for warm in (0, 1):
        o, wo = _opts(pkg, params, warm)
        a = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, nz)
        b = twin_noise_drive(twin, params, waypoints, car[:, perm], STEPS, o, wo, nz[:, perm], pad=2)
        for k in NH.KEYS:
            assert a[k][..., perm].tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
        c = twin_noise_drive(twin, params, waypoints, twins, STEPS, o, wo, nz2)
        for k in NH.KEYS:
            assert np.ascontiguousarray(c[k][..., 0]).tobytes() == np.ascontiguousarray(c[k][..., 1]).tobytes(), k
        assert not np.array_equal(c["seen"][..., 0], c["seen"][..., 2]) and not np.array_equal(c["car"][:, 0], c["car"][:, 2])


def _z(pkg, nz, steps):
    """[steps, 7, B]: mpc_drive_noise_draw of every car's seed at every message"""
    return np.array([[pkg.drive_noise_draw(s, t) for s in nz[SEED]] for t in range(steps)]).transpose(0, 2, 1)


def test_sensing_rule(pkg, twin, pop, waypoints):
    """seen == hist[:, 0:4] + sigma * z with z from mpc_drive_noise_draw, to the last bit (the rounded sum of the rounded product);
    rows with sigma = 0 are equal; the speed row is max(0, .), clamped for a car started at 0.01 mph with sigma_speed = 1; the window,
    hist row 12, is the TRUE car's; rows 8 / 9 are what the handler believed: they move with the noise."""
    params, car = pop
    car = car.copy(); car[3, 2] = 0.01
    nz = NH.noise_columns(B7, {POS: 0.3, PSI: 0.02, SPEED: 1.0})
    nz[POS, 4] = 0.0; nz[PSI, 5] = 0.0; nz[SPEED, 6] = 0.0
    cand = np.arange(9000, 9064)              # car 2's seed: the first of these whose first speed draw is below -0.1 (numpy's statement of it)
    nz[SEED, 2] = cand[np.argmax(NH.np_draw(cand, np.zeros(64, dtype=np.int64))[0][NH.Z_SPEED] < -0.1)]
    o, wo = _opts(pkg, params, 0)
    r = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, nz)
    z = _z(pkg, nz, STEPS)
    true = r["hist"][:, 0:4]
    want = true.copy()
    want[:, 0] = true[:, 0] + nz[POS] * z[:, NH.Z_X]; want[:, 1] = true[:, 1] + nz[POS] * z[:, NH.Z_Y]
    want[:, 2] = true[:, 2] + nz[PSI] * z[:, NH.Z_PSI]
    want[:, 3] = np.maximum(0.0, true[:, 3] + nz[SPEED] * z[:, NH.Z_SPEED])
    assert r["seen"].tobytes() == want.tobytes()
    assert np.array_equal(r["seen"][:, 0:2, 4], true[:, 0:2, 4]) and np.array_equal(r["seen"][:, 2, 5], true[:, 2, 5]) and np.array_equal(r["seen"][:, 3, 6], true[:, 3, 6])
    assert (r["seen"][:, 3, 2] == 0.0).any() and (r["seen"][:, 3] >= 0.0).all()          # (car 2: a reading below 0 became 0)
    assert np.array_equal(r["hist"][:, D.REC_K], D.twin_window(D.load_drive_twin(), waypoints, true[:, 0].ravel(), true[:, 1].ravel()).reshape(STEPS, B7))
    quiet = twin_noise_drive(twin, params, waypoints, car, 1, o, wo, None)
    assert not np.array_equal(r["hist"][0, D.REC_CTE], quiet["hist"][0, D.REC_CTE])
    # the acting rows alone leave what the handler is told alone
    act = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, NH.noise_columns(B7, {STEER: 0.01, DRIFT: 0.3, DROP: 0.5}))
    assert np.array_equal(act["seen"], act["hist"][:, 0:4])


def test_acting_and_dropping_rules(pkg, twin, pop, waypoints):
    """The plant between two messages is the plant under the column bias + sigma_steer z_steer, drift + sigma_drift z_drift (on the
    default column and on a car's own), bitwise against tests/drive_twin's plant.  p_drop = 1: rows 4 / 5 of every record are the
    initial command and rows 6 / 7 still vary; p_drop = 0 never drops; in between the dropped messages are those with u_drop < p."""
    params, car = pop
    o, wo = _opts(pkg, params, 0)
    dt = D.load_drive_twin()
    base = pkg.drive_plant_default(params, B7)
    own = DP.draw_plant(B7)
    for plant, col in ((None, base), (own, own)):
        nz = NH.noise_columns(B7, {STEER: 0.01, DRIFT: 0.3, DROP: 0.4})
        nz[STEER, 3] = 0.0; nz[DRIFT, 4] = 0.0
        r = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, nz, plant=plant)
        z = _z(pkg, nz, STEPS)
        dropped = z[:, NH.U_DROP] < nz[DROP]
        assert dropped.any() and not dropped.all()
        after = np.concatenate([r["hist"][1:, 0:6], r["car"][None]])
        for t in range(STEPS):
            pc = col.copy()
            pc[2] = col[2] + nz[STEER] * z[t, NH.Z_STEER]; pc[5] = col[5] + nz[DRIFT] * z[t, NH.Z_DRIFT]
            cmd = np.where(dropped[t], np.nan, r["hist"][t, 6:8])
            moved, ok = D.twin_plant_call(dt, params, r["hist"][t, 0:6], cmd, o, plant=pc)
            assert ok.all() and moved.tobytes() == np.ascontiguousarray(after[t]).tobytes(), t
            assert np.array_equal(after[t][4:6, dropped[t]], r["hist"][t, 4:6][:, dropped[t]])
    always = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, NH.noise_columns(B7, {DROP: 1.0}))
    assert (always["hist"][:, 4:6] == car[None, 4:6]).all() and np.array_equal(always["car"][4:6], car[4:6])
    # (the reply that was sent is still recorded: the steering reply of every car varies over the messages; these cars are far below
    # their target speed, so every throttle reply is the limit itself)
    assert (np.ptp(always["hist"][:, 6], axis=0) > 0).all() and np.isfinite(always["hist"]).all()
    assert not np.array_equal(always["hist"][:, 7], always["hist"][:, 5])
    never = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, NH.noise_columns(B7, {DROP: 0.0, DRIFT: 1e-300}))
    quiet = twin_noise_drive(twin, params, waypoints, car, STEPS, o, wo, None)
    assert np.array_equal(never["hist"][1:, 4], quiet["hist"][:-1, 6] * params.max_steering) and np.array_equal(never["hist"][1:, 5], quiet["hist"][:-1, 7])


def test_unusable_columns(pkg, twin, golden_dir, waypoints):
    """Each row not-a-number and infinite, sigma = -1, p_drop = 1.5 and -0.1, seed 0.5, -1 and 2^53, one per car among clean cars
    (noise_helpers.UNUSABLE): the rule of include/mpc_amd_noise.h, cold and warm."""
    params = BH.fast_params(pkg, golden_dir)
    car, clean, dirty, bad, zeroed = NH.child_cases(pkg, params, waypoints)
    assert len(bad) == len(NH.UNUSABLE) == 24
    for warm in (0, 1):
        o, wo = _opts(pkg, params, warm)
        ref, got, zero = (twin_noise_drive(twin, params, waypoints, car, 3, o, wo, nz, pad=1) for nz in (clean, dirty, zeroed))
        NH.check_unusable(got, ref, zero, bad, got["handler_status"])
        assert (zero["hist"][:, 10][:, bad] == NH.SUCCESS).sum() > 60       # (the rule is exercised: those steps became INFEASIBLE)


def _declared(header, name):
    found = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, re.M | re.S)
    assert found, name
    return [" ".join(q.split()) for q in found.group(1).split(",")]


def test_declarations_and_host_only_abi(pkg):
    """Each _noise form is its _budget form plus `const double *noise` behind `plant` and `double *seen` behind `hist`: declared in
    include/mpc_amd_noise.h, which mpc_amd.h includes, exported, bound with those argtypes; a NULL handle gives -1.
    mpc_drive_noise_default and mpc_drive_noise_draw need no device and refuse what they must.  The constants as a C compiler sees
    them; the ABI version and MpcDriveOpts stay."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    inc = os.path.join(_abi.ROOT, "include")
    assert '#include "mpc_amd_noise.h"' in open(os.path.join(inc, "mpc_amd.h")).read()
    noise_h, budget_h = open(os.path.join(inc, "mpc_amd_noise.h")).read(), open(os.path.join(inc, "mpc_amd_budget.h")).read()
    assert set(re.findall(r"^int\s+(mpc_[a-z0-9_]+)\s*\(", noise_h, re.M)) == set(_abi.NOISE_EXPORTS)
    for f in ("mpc_drive_batch_device", "mpc_drive_batch_device_fused", "mpc_drive_batch_host"):
        name, base = f + "_noise", _declared(budget_h, f + "_budget")
        assert hasattr(lib, name), name
        got = _declared(noise_h, name)
        ap, ah = base.index("const double *plant"), base.index("double *hist")
        assert got == base[:ap + 1] + ["const double *noise"] + base[ap + 1:ah + 1] + ["double *seen"] + base[ah + 1:], (name, got)
        bt, nt = list(getattr(lib, f + "_budget").argtypes), list(getattr(lib, name).argtypes)
        assert nt == bt[:ap + 1] + [C.c_void_p] + bt[ap + 1:ah + 1] + [C.c_void_p] + bt[ah + 1:], name
        args = [None if "*" in q else 0 for q in got]
        assert getattr(lib, name)(*args) == -1 and b"NULL handle" in lib.mpc_last_error(), name
    assert _declared(noise_h, "mpc_drive_noise_default") == ["double *col7"]
    assert _declared(noise_h, "mpc_drive_noise_draw") == ["double seed", "int32_t step", "double *out7"]
    assert _declared(noise_h, "mpc_debug_philox4x32") == ["const uint32_t ctr[4]", "const uint32_t key[2]", "uint32_t out[4]"]
    assert _declared(noise_h, "mpc_debug_drive_noise_device") == ["MpcHandle *h", "int64_t n", "const double *seed", "const int32_t *step", "double *out", "void *stream"]
    assert lib.mpc_abi_version() == 5
    col = np.full(8, NH.SENTINEL)
    assert lib.mpc_drive_noise_default(col.ctypes.data) == 0 and col.tolist() == [0.0] * 7 + [NH.SENTINEL]
    assert lib.mpc_drive_noise_default(None) == -1 and b"NULL" in lib.mpc_last_error()
    assert np.array_equal(pkg.drive_noise_default(), np.zeros(7)) and pkg.drive_noise_default(3).shape == (7, 3)
    assert np.array_equal(pkg.BatchedMPC.drive_noise_default(seeds=[5, 2 ** 53 - 1])[0], [5.0, 2.0 ** 53 - 1])
    for seeds in ([-1, 0], [0.5, 1.0], [2 ** 53, 0]):
        with pytest.raises(ValueError):
            pkg.drive_noise_default(2, seeds)
    out = np.full(8, NH.SENTINEL)
    for seed, step in ((0.5, 0), (-1.0, 0), (2.0 ** 53, 0), (np.nan, 0), (np.inf, 0), (1.0, -1), (1.0, -2 ** 31)):
        assert lib.mpc_drive_noise_draw(C.c_double(seed), C.c_int32(step), out.ctypes.data) == -1 and (out == NH.SENTINEL).all(), (seed, step)
    assert lib.mpc_drive_noise_draw(C.c_double(1.0), C.c_int32(0), None) == -1
    assert lib.mpc_drive_noise_draw(C.c_double(2.0 ** 53 - 1), C.c_int32(2 ** 31 - 1), out.ctypes.data) == 0 and np.isfinite(out[:7]).all() and out[7] == NH.SENTINEL
    assert lib.mpc_debug_drive_noise_device(None, 1, None, None, None, None) == -1 and b"NULL handle" in lib.mpc_last_error()
    names = "MPC_NNOISE MPC_NOISE_SEED MPC_NOISE_POS MPC_NOISE_PSI MPC_NOISE_SPEED MPC_NOISE_STEER MPC_NOISE_DRIFT MPC_NOISE_DROP MPC_DRAW_U_DROP MPC_DRIVE_REC".split()
    src = '#include <stdio.h>\n#include "mpc_amd.h"\nint main(){printf("%s\\n", (int)sizeof(MpcDriveOpts), %s);return 0;}\n' % (" ".join(["%d"] * (len(names) + 1)), ", ".join(names))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", inc, "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        assert [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()] == [C.sizeof(_abi.MpcDriveOpts), 7, 0, 1, 2, 3, 4, 5, 6, 6, 13]
    assert (_abi.NNOISE, _abi.NOISE_SEED, _abi.NOISE_DROP, _abi.DRAW_U_DROP) == (7, 0, 6, 6)


class _Handle:
    """drive_numpy's argument checks come before anything touches the handle"""
    _h = None


def test_python_layer_argument_errors(pkg, pop, waypoints):
    """drive_numpy(noise=...) with a wrong shape or dtype raises ValueError before the library is called"""
    params, car = pop
    tx, ty = D.track_of(waypoints)
    for bad in (np.zeros((6, B7)), np.zeros((7, B7 + 1)), np.zeros(7), np.zeros((7, B7), dtype=np.float32), np.zeros((7, B7), dtype=np.int64)):
        with pytest.raises(ValueError, match="noise"):
            pkg.BatchedMPC.drive_numpy(_Handle(), car, tx, ty, 2, noise=bad)


def test_sanitized_program(golden_dir):
    """tests/cpp/drive_noise_sanitize.cpp: a stand-alone program around the CPU build and mpc_params.cpp, compiled with
    -fsanitize=address,undefined and run directly (no preload anywhere); its input includes columns that cannot be used."""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "carnd-mpc-project_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drive_noise_sanitize")
        subprocess.check_call(["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "cpp", "drive_noise_sanitize.cpp"), NH.TWIN_SRC,
                                                                   os.path.join(ROOT, "carnd-mpc-project_amd", "csrc", "mpc_params.cpp"), "-lm", "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, os.path.join(golden_dir, "config-fast.json")], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rows = re.findall(r"^warm (\d) status((?: \d+){5})$", p.stdout, re.M)
    assert [r[0] for r in rows] == ["0", "1"] and "bad 0" in p.stdout, p.stdout
    for _, line in rows:
        assert [int(v) for v in line.split()] == [0, 0, 3, 3, 0], p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
