"""Every batch entry point of include/mpc_amd.h in every form, through the raw C ABI (test infrastructure; shared by
tests/test_entry_points_gpu.py and tools/entry_point_dump.py).  The header's rule is written down once more here, independently of
the binding: a family's arguments, `model` behind its inputs in the _model forms, the warm arguments behind that in the _warm forms.

call() makes one call with leading dimensions of its choice: every input holds NaN from column B on, every output a sentinel
everywhere, and the result says whether anything from column B on was touched."""
import ctypes as C

import numpy as np

F, I = -7777.25, -12345          # what every output array holds before a call
NPTS = 6
EXTRA_LATENCY = 0.02
STEPS = 3
FORMS = ("", "_model", "_warm", "_warm_model")
WARM_ARGS = "warm_in warm_status warm_out ld_warm opts"

# family -> (the plain form's arguments, "|" where the _model and _warm forms put theirs; what its _warm forms bring)
FAMILIES = {
    "mpc_solve_batch_device": ("h B ld state coeffs yaw_lo yaw_hi weights | out traj status iters stream", WARM_ARGS),
    "mpc_solve_batch_host": ("h B ld state coeffs yaw_lo yaw_hi weights | out traj status iters", WARM_ARGS),
    "mpc_run_batch_device": ("h B ld npts pose ptsx ptsy | out8 traj status iters pre stream", WARM_ARGS),
    "mpc_run_batch_host": ("h B ld npts pose ptsx ptsy | out8 traj status iters pre", WARM_ARGS),
    "mpc_telemetry_batch_device": ("h B ld npts tel extra ptsx ptsy | cmd out8 status stream", WARM_ARGS),
    "mpc_telemetry_batch_host": ("h B ld npts tel extra ptsx ptsy | cmd status", WARM_ARGS),
    "mpc_wire_telemetry_batch_host": ("h B frames prev_throttle extra | cmd status", WARM_ARGS),
    "mpc_rollout_batch_device": ("h B ld steps state coeffs yaw_lo yaw_hi weights | hist status iters stream", "opts"),
    # two forms only: warm_start and opts are arguments of both
    "mpc_rollout_batch_device_fused": ("h B ld steps state coeffs yaw_lo yaw_hi weights | warm_start opts hist status iters stream", None),
}
SOLVE = ("mpc_solve_batch_device", "mpc_solve_batch_host")
RUN = ("mpc_run_batch_device", "mpc_run_batch_host")
TELEMETRY = ("mpc_telemetry_batch_device", "mpc_telemetry_batch_host")
ROLLOUT = ("mpc_rollout_batch_device", "mpc_rollout_batch_device_fused")
WIRE = "mpc_wire_telemetry_batch_host"
DEVICE = tuple(f for f in FAMILIES if "stream" in FAMILIES[f][0])
HOST = tuple(f for f in FAMILIES if f not in DEVICE)

INPUTS = ("state", "coeffs", "yaw_lo", "yaw_hi", "weights", "pose", "tel", "ptsx", "ptsy", "model", "warm_in", "warm_status", "prev_throttle")
INT_ARRAYS = ("status", "iters", "warm_status")
INT_SCALARS = ("npts", "steps", "warm_start")


def forms_of(family):
    return FORMS if FAMILIES[family][1] else FORMS[:2]


def arguments(family, form):
    """the argument names of `family`'s `form`, in the order of the declaration"""
    head, tail = FAMILIES[family][0].split(" | ")
    warm = FAMILIES[family][1].split() if "_warm" in form else []
    return head.split() + (["model"] if "_model" in form else []) + warm + tail.split()


def cars(pkg, params, waypoints, B):
    """B lake-track cars with everything any family takes: the solve's inputs, run()'s pose and waypoints, the telemetry rows, a
    model column per car (values around the handle's own) and the handle's weights in every column."""
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=77)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    d = {k: f(sc[k]) for k in ("state", "coeffs", "yaw_lo", "yaw_hi", "pose", "ptsx", "ptsy")}
    assert d["ptsx"].shape[0] == NPTS
    pose = d["pose"]
    d["tel"] = f(np.stack([pose[0], pose[1], pose[2], pose[3] * 3600.0 / 1609.34, -pose[4], np.full(B, 0.3)]))
    rng = np.random.default_rng(9)
    own = np.array([[getattr(params, k)] for k in ("dt", "Lf", "max_steering", "max_acceleration", "max_deceleration", "max_speed")])
    d["model"] = f(own * rng.uniform(0.9, 1.1, (6, B)))
    d["weights"] = f(np.repeat(np.array(list(params.weights))[:12, None], B, axis=1))
    d["prev_throttle"] = f(d["tel"][5])
    return d


def call(pkg, mpc, dev, family, form, d, ld=None, ld_warm=None, rec=None, hist=True, warm_start=0, opts=None, null_model=False,
         over=None, B=None, width=None):
    """One call of `family` + `form` on the handle `mpc` for the cars `d`.  ld / ld_warm: the leading dimensions (default B).  rec: the
    result of an earlier call whose warm buffer and status this one starts from (None: warm_in = warm_status = NULL).  null_model: a
    _model form with model = NULL.  over: arguments replaced by name after everything else is in place (None: a NULL pointer) -- the
    arrays are `width` columns wide whatever ld and ld_warm say (default: exactly ld and ld_warm).
    -> {"rc", "msg", "pad", name: array cut to B columns for every array the call may write}."""
    import torch
    lib = pkg.library()
    nB = d["state"].shape[1]
    B = nB if B is None else B
    ld = B if ld is None else ld
    ld_warm = B if ld_warm is None else ld_warm
    wide, wide_warm = (max(ld, B, nB), max(ld_warm, B, nB)) if width is None else (width, width)
    device = family in DEVICE
    N, wrows = mpc.N, mpc.warm_rows()
    rows = {"state": 6, "coeffs": 5, "weights": 12, "pose": 6, "tel": 6, "ptsx": NPTS, "ptsy": NPTS, "model": 6, "out": 9, "traj": 2 * N,
            "out8": 8, "pre": 15, "cmd": 2, "hist": STEPS * 9, "warm_in": wrows, "warm_out": wrows}
    names = arguments(family, form)
    arrays, keep = {}, {}
    for name in names:
        if name in ("h", "B", "ld", "ld_warm", "extra", "opts", "stream", "frames") or name in INT_SCALARS:
            continue
        # (the warm buffers have ld_warm; the wire form has no ld: its other arrays are B wide)
        stride = wide_warm if name in ("warm_in", "warm_out") else (wide if family != WIRE else nB)
        shape = (rows[name], stride) if name in rows else (stride,)
        a = np.full(shape, I, dtype=np.int32) if name in INT_ARRAYS else np.full(shape, F)
        if name in INPUTS:
            src = d.get(name)
            if name in ("warm_in", "warm_status"):
                src = None if rec is None else rec["warm_out" if name == "warm_in" else "status"]
            if src is None or (name == "model" and null_model):
                arrays[name] = None
                continue
            if a.dtype != np.int32:
                a[...] = np.nan
            a[..., :nB] = src
        arrays[name] = a
    if "hist" in arrays and not hist:
        arrays["hist"] = None
    frames = None
    if "frames" in names:
        frames = (pkg.MpcWireTelemetry * nB)()
        for i in range(nB):
            t = d["tel"][:, i]
            frames[i].x, frames[i].y, frames[i].psi, frames[i].speed, frames[i].steering_angle, frames[i].throttle = t
            frames[i].npts = NPTS
            for q in range(NPTS):
                frames[i].ptsx[q] = d["ptsx"][q, i]; frames[i].ptsy[q] = d["ptsy"][q, i]
    before = {k: a.copy() for k, a in arrays.items() if a is not None}
    if device:
        arrays = {k: (torch.from_numpy(a).to(dev) if a is not None else None) for k, a in arrays.items()}
        keep = arrays
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr() if device else a.ctypes.data)
    scalars = {"h": mpc._h, "B": C.c_int64(B), "ld": C.c_int64(ld), "ld_warm": C.c_int64(ld_warm), "extra": C.c_double(EXTRA_LATENCY),
               "npts": C.c_int(NPTS), "steps": C.c_int(STEPS), "warm_start": C.c_int(warm_start),
               "opts": C.byref(opts) if opts is not None else None, "frames": frames,
               "stream": C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if device else None}
    args = {name: scalars[name] if name in scalars else ptr(arrays[name]) for name in names}
    for name, v in (over or {}).items():
        if name in args:
            args[name] = None if v is None else (C.c_int(v) if name in INT_SCALARS else C.c_int64(v))
    rc = getattr(lib, family + form)(*[args[name] for name in names])
    if device:
        torch.cuda.synchronize()
    res = {"rc": rc, "msg": lib.mpc_last_error().decode() if rc != 0 else "", "pad": True}
    for name, a0 in before.items():
        a = keep[name].cpu().numpy() if device else arrays[name]
        bits = np.uint32 if a.dtype == np.int32 else np.uint64
        res["pad"] = res["pad"] and bool(np.array_equal(a[..., nB:].view(bits), a0[..., nB:].view(bits)))
        if name not in INPUTS or name in ("ptsx", "ptsy") or (name == "state" and family in ROLLOUT):
            res[name] = np.ascontiguousarray(a[..., :nB])
    return res


def empty_call(pkg, mpc, family, form):
    """B = 0 with every array NULL (the scalars a form checks before it looks at B are valid) -> (rc, text)"""
    lib = pkg.library()
    vals = {"h": mpc._h, "B": C.c_int64(0), "ld": C.c_int64(0), "ld_warm": C.c_int64(0), "extra": C.c_double(EXTRA_LATENCY),
            "npts": C.c_int(NPTS), "steps": C.c_int(STEPS), "warm_start": C.c_int(1)}
    rc = getattr(lib, family + form)(*[vals.get(name) for name in arguments(family, form)])
    return rc, lib.mpc_last_error().decode() if rc != 0 else ""


def sequence(pkg, mpc, dev, family, form, d, null_model=False, **kw):
    """What a form is called with at a shape: once, and a warm form once more from the buffer and status the first call wrote (the
    fused rollout: cold and with warm_start = 1).  -> the results, in order."""
    if family == "mpc_rollout_batch_device_fused":
        return [call(pkg, mpc, dev, family, form, d, warm_start=w, null_model=null_model, **kw) for w in (0, 1)]
    first = call(pkg, mpc, dev, family, form, d, null_model=null_model, **kw)
    if "_warm" not in form or family in ROLLOUT or first["rc"] != 0:
        return [first]
    return [first, call(pkg, mpc, dev, family, form, d, rec=first, null_model=null_model, **kw)]


# ---- refusals: (handle, families, forms, how the call differs, expected code, substring of mpc_last_error()) --------------------------
INVALID, UNSUPPORTED = -1, -4
ALL = tuple(FAMILIES)
WITH_WARM_BUFFER = tuple(f for f in ALL if f not in ROLLOUT)
MODEL_FORMS, WARM_ONLY, WARM_FORMS, COLD_FORMS = ("_model", "_warm_model"), ("_warm",), ("_warm", "_warm_model"), ("", "_model")
BAD_SIZE, BAD_MU = {"size": 8}, {"mu_init": 0.2}
REFUSALS = [
    ("f32", ALL, MODEL_FORMS, {}, INVALID, "per-instance model values: fp64 handles only"),
    ("f32", ALL, WARM_ONLY, {}, INVALID, "warm start: fp64 handles only"),
    ("f32", SOLVE, ("",), {}, INVALID, "other precision"),
    ("f32", ("mpc_run_batch_host",), ("",), {}, INVALID, "run() entry points are fp64 only"),
    ("n25", ALL, WARM_ONLY, {}, UNSUPPORTED, "f64_f32_start = 0"),
    ("n25", ALL, MODEL_FORMS, {}, 0, ""),
    ("soc", ALL, WARM_FORMS, {}, UNSUPPORTED, "max_soc"),
    ("soc", ALL, COLD_FORMS, {}, 0, ""),
    ("fast", ALL, WARM_FORMS, {"opts": BAD_SIZE}, INVALID, "MpcWarmOpts.size"),
    ("fast", ALL, WARM_FORMS, {"opts": BAD_MU}, INVALID, "MpcWarmOpts:"),
    ("fast", WITH_WARM_BUFFER, WARM_FORMS, {"ld_warm": 15}, INVALID, "ld_warm"),
    ("fast", RUN + TELEMETRY, FORMS, {"npts": 2}, INVALID, "npts"),
    ("fast", ROLLOUT, FORMS, {"steps": 0}, INVALID, "steps < 1"),
    ("fast", ("mpc_solve_batch_device",), FORMS, {"ld": 15}, INVALID, "ld < B"),
    ("fast", ("mpc_solve_batch_host",), FORMS, {"ld": 15}, INVALID, "bad B/ld"),
    ("fast", RUN + TELEMETRY + ROLLOUT, FORMS, {"ld": 15}, INVALID, "bad B/ld"),
    ("fast", ("mpc_solve_batch_device",), FORMS, {"B": 17}, INVALID, "max_batch"),
    ("fast", ("mpc_solve_batch_host",), FORMS, {"B": 17}, INVALID, "bad B/ld"),
    ("fast", ("mpc_run_batch_device",), FORMS, {"out8": None}, INVALID, "NULL argument"),
    ("fast", ("mpc_telemetry_batch_device",), FORMS, {"cmd": None}, INVALID, "NULL argument"),
    # precedence: the handle before the options, max_soc before the options, the options before a family's own NULL test
    ("f32", ALL, WARM_ONLY, {"opts": BAD_SIZE}, INVALID, "warm start: fp64 handles only"),
    ("f32", ALL, ("_warm_model",), {"opts": BAD_SIZE}, INVALID, "per-instance model values: fp64 handles only"),
    ("soc", ALL, WARM_FORMS, {"opts": BAD_SIZE}, UNSUPPORTED, "max_soc"),
    ("fast", ("mpc_run_batch_device",), WARM_FORMS, {"out8": None, "opts": BAD_SIZE}, INVALID, "MpcWarmOpts.size"),
]
HANDLES = {"fast": {}, "f32": {"precision": 1}, "n25": {"N": 25}, "soc": {"max_soc": 4}}
B16 = 16


def refusal_calls(pkg, mpc, dev, d, handle):
    """Every row of REFUSALS for `handle` on every form it applies to -> [(label, rc, text, expected rc, expected substring)].  A
    warm form brings a warm buffer of the right size (the first call's, where one was served); the fused rollout's warm forms are its
    two forms with warm_start = 1."""
    out = []
    for row, (hname, families, forms, how, want_rc, want_text) in enumerate(REFUSALS):
        if hname != handle:
            continue
        for family in families:
            for form in forms:
                kw = {"width": 24}
                if family == "mpc_rollout_batch_device_fused":      # _warm -> fused with warm_start = 1, _warm_model -> fused_model with it
                    kw["warm_start"] = 1 if "_warm" in form else 0
                    form = form.replace("_warm", "")
                elif form not in forms_of(family):
                    continue
                how_ = dict(how)
                if "opts" in how_:
                    kw["opts"] = pkg.warm_opts_default(**how_.pop("opts"))
                if "B" in how_:
                    kw["B"] = how_.pop("B")
                if "_warm" in form and family not in ROLLOUT:   # (a warm buffer comes with the call, no column of it valid: with NULL arrays nobody looks at ld_warm)
                    kw["rec"] = {"warm_out": np.zeros((mpc.warm_rows(), B16)), "status": np.ones(B16, dtype=np.int32)}
                r = call(pkg, mpc, dev, family, form, d, over=how_, **kw)
                label = "row %d %s %s%s%s" % (row, hname, family, form, " warm_start=1" if kw.get("warm_start") else "")
                out.append((label, r["rc"], r["msg"], want_rc, want_text))
    return out


def differing_words(a, b):
    """(words compared, words that differ) between two results of call(): every array of either, bit for bit"""
    n = bad = 0
    for k in sorted(set(a) | set(b)):
        if k in ("rc", "msg", "pad"):
            continue
        x, y = a.get(k), b.get(k)
        if x is None or y is None or x.shape != y.shape:
            size = max(0 if x is None else x.size, 0 if y is None else y.size)
            n += size; bad += size
            continue
        bits = np.uint32 if x.dtype == np.int32 else np.uint64
        n += x.size; bad += int((x.view(bits) != y.view(bits)).sum())
    return n, bad


def with_params(params, **kw):
    q = params.copy()
    for k, v in kw.items():
        setattr(q, k, v)
    return q
