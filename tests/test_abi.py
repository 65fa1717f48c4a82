"""The C ABI (include/mpc_amd.h): the library loads, exports every declared symbol, parameter loading
matches the oracle's Config::load restatement, and compute entry points FAIL LOUDLY without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O


def test_library_exports_every_declared_symbol(pkg):
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    header = open(os.path.join(_abi.ROOT, "include", "mpc_amd.h")).read()
    declared = set(re.findall(r"\b(mpc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_abi.EXPORTS), declared ^ set(_abi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mpc_abi_version() == _abi.ABI_VERSION


def test_struct_layout_matches_header(pkg):
    """sizeof(MpcParams) seen by ctypes == the C compiler's (via a tiny compiled probe)."""
    import subprocess, tempfile
    from carnd_mpc_project_amd import _abi
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mpc_amd.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(MpcParams), offsetof(MpcParams, tol), offsetof(MpcParams, steers), sizeof(MpcBatchStats));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(_abi.ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")])
        out = subprocess.check_output([os.path.join(d, "p")]).split()
    assert int(out[0]) == C.sizeof(pkg.MpcParams)
    assert int(out[1]) == pkg.MpcParams.tol.offset
    assert int(out[2]) == pkg.MpcParams.steers.offset
    assert int(out[3]) == C.sizeof(pkg.MpcBatchStats)


@pytest.mark.parametrize("name", ["config-stable.json", "config-fast.json", "config-no-latency.json"])
def test_params_from_json_match_oracle_config(pkg, golden_dir, name):
    p = pkg.params_from_json(os.path.join(golden_dir, name))
    c = O.load_config(name)
    assert (p.N, p.dt, p.Lf) == (c.N, c.dt, c.Lf)
    for f_abi, f_orc in (("max_steering", "max_steering"), ("max_acceleration", "max_acceleration"),
                         ("max_deceleration", "max_deceleration"), ("max_speed", "max_speed"),
                         ("cte_panic", "cte_panic"), ("epsi_panic", "epsi_panic"), ("lookahead", "lookahead"),
                         ("max_fit_error", "max_fit_error"), ("steer_adj_thresh", "steer_adj_thresh"),
                         ("steer_adj_ratio", "steer_adj_ratio")):
        assert getattr(p, f_abi) == getattr(c, f_orc), f_abi
    assert p.max_fit_order == c.max_fit_order and p.latency_ms == c.latency
    assert list(p.weights) == list(c.weights)[:12]
    assert (p.n_steers, p.n_steer_speeds, p.n_yaw_changes, p.n_yaw_change_speeds) == (c.n_steers, c.n_steer_speeds, c.n_yaw_changes, c.n_yaw_change_speeds)
    assert list(p.steers)[:p.n_steers] == list(c.steers)[:c.n_steers]
    assert list(p.steer_speeds)[:p.n_steer_speeds] == list(c.steer_speeds)[:c.n_steer_speeds]
    assert list(p.yaw_change_speeds)[:p.n_yaw_change_speeds] == list(c.yaw_change_speeds)[:c.n_yaw_change_speeds]
    assert p.branch_mode == 0 and p.precision == 0 and p.tol == 1e-8
    assert p.lane_compact == -1 and p.tail_cut == 0 and p.f32_finish == 1 and p.f64_f32_start == 2 and p.initial_state_rows == 0 and p.wave_max_batch == 0 and p.f32_phase_refill == 0


def test_params_errors(pkg, tmp_path):
    with pytest.raises(pkg.MpcError):
        pkg.params_from_json(str(tmp_path / "missing.json"))
    bad = tmp_path / "bad.json"
    bad.write_text('{"N": 10, "dt": 0.1, "weights": [1, 2, 3]}')     # Config.cpp:61 assert(weights.size() > 11)
    with pytest.raises(pkg.MpcError):
        pkg.params_from_json(str(bad))
    d = pkg.params_default()                                          # Config.cpp:5-29
    assert d.N == 25 and d.dt == 0.025 and d.n_steers == 3 and d.n_steer_speeds == 4


def test_no_cpu_fallback_without_gpu(pkg, golden_dir):
    """On a box without a gfx950 device the product must fail loudly, not compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    p = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"))
    with pytest.raises(pkg.MpcError) as e:
        pkg.BatchedMPC(p, 16)
    assert "NO_DEVICE" in str(e.value) or "HIP" in str(e.value)


def test_invalid_params_rejected(pkg, golden_dir):
    p = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"))
    h = C.c_void_p()
    for field, val in (("N", 2), ("N", 65), ("abi_version", 99), ("branch_mode", 1), ("precision", 7), ("max_iter", 0), ("lane_compact", 8),
                       ("lane_compact", -2)):
        q = p.copy(); setattr(q, field, val)
        rc = pkg.library().mpc_create(C.byref(q), 0, 16, C.byref(h))
        assert rc in (-1, -4), (field, rc)


TERMINATION_TOLS = ("dual_inf_tol", "constr_viol_tol", "compl_inf_tol", "acceptable_tol", "acceptable_dual_inf_tol",
                    "acceptable_constr_viol_tol", "acceptable_compl_inf_tol", "mixed_switch_mu")


def _create_rc(pkg, q):
    """mpc_create's return code and text for `q`.  validate_params runs before the device is looked up: on a machine without a GPU
    accepted parameters give MPC_ERR_NO_DEVICE (-2), refused ones MPC_ERR_INVALID (-1); with one, 0 (the handle is destroyed)."""
    h = C.c_void_p()
    rc = pkg.library().mpc_create(C.byref(q), 0, 16, C.byref(h))
    err = pkg.library().mpc_last_error() or b""
    if rc == 0:
        pkg.library().mpc_destroy(h)
    return rc, err.decode()


@pytest.mark.parametrize("field", TERMINATION_TOLS)
@pytest.mark.parametrize("value", [0.0, -1e-4, float("nan")])
def test_termination_tolerances_must_be_positive(pkg, golden_dir, field, value):
    """The termination fields of ABI 4 and mixed_switch_mu: zero (an MpcParams that mpc_params_default never filled), negative or
    not a number is MPC_ERR_INVALID with a text that names the field -- with them every instance would run to MPC_STATUS_MAXITER."""
    q = pkg.params_from_json(os.path.join(golden_dir, "config-stable.json"))
    setattr(q, field, value)
    rc, err = _create_rc(pkg, q)
    assert rc == -1, (field, value, rc, err)
    assert re.search(r"\b%s\b" % field, err), (field, err)


def test_termination_fields_left_zero_are_refused_and_the_shipped_ones_accepted(pkg, golden_dir):
    """A struct zeroed apart from what validate_params checked before ABI 4's fields is refused; acceptable_iter < 0 is refused, 0
    ("off") is not; mpc_params_default and the three golden configs pass (-2 without a device, never -1)."""
    import torch
    accepted = (0,) if torch.cuda.is_available() else (-2,)
    good = [pkg.params_default()] + [pkg.params_from_json(os.path.join(golden_dir, n))
                                     for n in ("config-stable.json", "config-fast.json", "config-no-latency.json")]
    for q in good:
        rc, err = _create_rc(pkg, q)
        assert rc in accepted, (rc, err)
    d = good[1]
    z = pkg.MpcParams()
    for f in ("abi_version", "N", "dt", "Lf", "max_speed", "max_steering", "n_steer_speeds", "max_iter", "tol"):
        setattr(z, f, getattr(d, f))
    rc, err = _create_rc(pkg, z)
    assert rc == -1 and "dual_inf_tol" in err, (rc, err)
    q = d.copy(); q.acceptable_iter = -1
    rc, err = _create_rc(pkg, q)
    assert rc == -1 and "acceptable_iter" in err, (rc, err)
    q.acceptable_iter = 0
    rc, err = _create_rc(pkg, q)
    assert rc in accepted, (rc, err)
    if not torch.cuda.is_available():
        q = d.copy(); q.mixed_switch_mu = 0.0
        assert _create_rc(pkg, q)[0] == -1 and _create_rc(pkg, d)[0] == -2      # refused before the device is looked up


@pytest.mark.parametrize("name", ["config-stable.json", "config-fast.json", "config-no-latency.json"])
def test_params_from_json_against_a_third_reader(pkg, golden_dir, name):
    """mpc_params.cpp and the oracle's reader are both purpose-built flat-JSON parsers (a shared mistake would pass the
    test above): here the file goes through Python's json module and Config::load's rules (src/utils/Config.cpp:31-87) are
    applied in numpy."""
    import json
    import numpy as np
    j = json.load(open(os.path.join(golden_dir, name)))
    mph = lambda x: x * 1609.34 / 3600.0                                  # utils.h:11-13
    p = pkg.params_from_json(os.path.join(golden_dir, name))
    assert (p.N, p.dt, p.latency_ms, p.max_fit_order) == (j["N"], j["dt"], j["latency"], j["max polynomial fitting order"])
    assert p.lookahead == pytest.approx(j["latency"] * 1e-3, abs=1e-15) and p.ipopt_timeout == j["ipopt timeout"]
    assert p.max_fit_error == j["max polynomial fitting error"] and p.Lf == j["Lf"]
    assert p.max_steering == pytest.approx(np.deg2rad(j["max steering"]), rel=1e-15)
    assert p.max_acceleration == pytest.approx(mph(j["max acceleration"]), rel=1e-15)
    assert p.max_deceleration == pytest.approx(mph(j["max deceleration"]), rel=1e-15)
    assert p.max_speed == pytest.approx(mph(j["max speed"]), rel=1e-15)
    assert (p.epsi_panic, p.cte_panic, p.steer_adj_thresh) == (j["epsi panic"], j["cte panic"], j["steer adjustment threshold"])
    assert p.steer_adj_ratio == min(max(j["steer adjustment ratio"], 0.0), 0.1)
    assert list(p.weights)[:12] == j["weights"][:12] and len(j["weights"]) > 11
    scale = mph(j["max speed"]) / mph(100)                                 # Config.cpp:65
    for key, tab, n_tab, skey, stab, n_stab in (("steers", p.steers, p.n_steers, "steer speeds", p.steer_speeds, p.n_steer_speeds),
                                                ("yaw changes", p.yaw_changes, p.n_yaw_changes, "yaw change speeds", p.yaw_change_speeds, p.n_yaw_change_speeds)):
        assert n_tab == len(j[key]) and list(tab)[:n_tab] == j[key]
        want = [mph(s) * scale if scale > 1 else min(mph(s), mph(j["max speed"])) for s in j[skey]]
        assert n_stab == len(want) and np.allclose(list(stab)[:n_stab], want, rtol=1e-15)


def test_inflight_advice(pkg, golden_dir):
    """mpc_inflight_advice: two devices' worth of lanes in flight, 2 .. 8 launches, at least 4 for two-launch solves and long
    horizons (what bench.py runs its workloads with)."""
    import os
    p = pkg.params_from_json(os.path.join(golden_dir, "config-fast.json"))
    assert pkg.inflight_advice(p, 65536) == 2 and pkg.inflight_advice(p, 4096) == 8 and pkg.inflight_advice(p, 32768) == 4 and pkg.inflight_advice(p, 16384) == 8
    q = p.copy(); q.precision = pkg.PRECISION_F32
    assert pkg.inflight_advice(q, 131072) == 4
    q = p.copy(); q.N = 25
    assert pkg.inflight_advice(q, 32768) == 4
    q = p.copy(); q.f64_f32_start = 1
    assert pkg.inflight_advice(q, 65536) == 4


BATCH_ENTRY = re.compile(r"mpc_(solve|run|telemetry|rollout|wire_telemetry)_batch")


def declared_parameters(name):
    """The parameter list of `name`'s declaration in include/mpc_amd.h (comments stripped: a mention there is no declaration)."""
    from carnd_mpc_project_amd import _abi
    header = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(_abi.ROOT, "include", "mpc_amd.h")).read(), flags=re.S)
    found = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % re.escape(name), header)
    assert len(found) == 1, (name, found)
    params = [" ".join(q.split()) for q in found[0].split(",")]
    return [] if params == ["void"] else params


def c_kind(param):
    """What ctypes has to pass for a declared parameter: "pointer", or the ctypes integer / floating type."""
    if "*" in param:
        return "pointer"
    return {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}[param.rsplit(" ", 1)[0].replace("const ", "")]


def test_argtypes_match_the_header(pkg):
    """Every argtypes list of the binding against the declaration it stands for: the same number of parameters and the same kind
    at each position (a wrong count corrupts the call silently).  Every batch entry point must have one."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    checked = 0
    for name in _abi.EXPORTS:
        params = declared_parameters(name)
        argtypes = getattr(lib, name).argtypes
        if BATCH_ENTRY.match(name):
            assert argtypes is not None, name
        if argtypes is None:
            continue
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (t, q) in enumerate(zip(argtypes, params)):
            kind = c_kind(q)
            if kind == "pointer":
                assert t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer), (name, i, q, t)
            else:
                assert t is kind, (name, i, q, t)
        checked += 1
    assert checked >= 36


def test_every_batch_entry_point_refuses_a_null_handle(pkg):
    """NULL handle, B = 0, NULL arrays: MPC_ERR_INVALID and a text from every form -- the handle is the first thing each checks, so
    no device is needed."""
    from carnd_mpc_project_amd import _abi
    lib = pkg.library()
    names = [n for n in _abi.EXPORTS if BATCH_ENTRY.match(n)]
    assert len(names) == 36      # 8 families x 4 forms, the fused rollout's 2, the fp32 solve's 2
    for name in names:
        fn = getattr(lib, name)
        args = [None if "*" in q else (0.0 if c_kind(q) is C.c_double else 0) for q in declared_parameters(name)]
        assert fn(*args) == -1, name
        err = lib.mpc_last_error()
        assert err and b"NULL" in err, (name, err)
