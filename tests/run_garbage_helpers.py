"""Helpers of the tests that feed run() and the telemetry handler inputs no caller should send (test infrastructure): the defect
lists, the TEST-ONLY CPU build of the whole path (mpc_twin_run of tests/host_twin) and the child process that runs it under a time
limit, so that a loop in the code under test fails a test instead of hanging the suite.  What the path owes a defective instance is
stated at include/mpc_amd.h (mpc_telemetry_batch_device): a status other than SUCCESS, a launch that ends, and clean neighbours that
come out bit for bit as in a clean batch."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = "config-fast.json"
NPTS = 6
EXTRA_LATENCY = 0.004
CHILD_TIMEOUT_S = 120          # the clean and the dirty batch together take about a second; a loop of 1.6e11 turns does not end in this
SEED = 83

# rows of tel: x, y, psi [rad], speed [mph], steering_angle, previous throttle;  rows of pose: x, y, psi, v, steering, acceleration
PSI_OUT_OF_RANGE = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("1e300", 1e300), ("1e12", 1e12), ("-1e9", -1e9)]
PSI_IN_RANGE = [("1e9 - 1", 1e9 - 1), ("200 pi + 0.3", 200 * np.pi + 0.3)]       # the last value fsincos takes; the closed-form region
MODEL_LF, MODEL_MAX_STEERING = 1, 2                                              # rows of model (MPC_MODEL_*)


def _f(a):
    return np.array(a, dtype=np.float64, copy=True, order="C")


def _waypoint_defects(x, px, py, row_x, row_y, row_psi, at_rest, straight):
    """the defects of the waypoint lists; x = tel or pose (rows 0, 1, 2 are x, y, psi in both); at_rest(i): the car of instance i does
    not move during the latency compensation, so that the waypoints put AT the car are at the pose run() sees; straight(i): it does
    not turn during it, so that the heading run() sees is the 0 written here"""
    n = px.shape[0]
    ahead = np.arange(1, n + 1, dtype=np.float64)

    def at_the_car(i):
        at_rest(i); px[:, i] = x[row_x, i]; py[:, i] = x[row_y, i]

    def one_x(i):                                   # heading 0: the vehicle-frame x of every waypoint is the same number
        straight(i); x[row_psi, i] = 0.0; px[:, i] = x[row_x, i] + 10.0; py[:, i] = x[row_y, i] + 0.5 * ahead

    def behind(i):                                  # heading 0, the waypoints at -5, -10, ... m: decreasing x, behind the car
        straight(i); x[row_psi, i] = 0.0; px[:, i] = x[row_x, i] - 5.0 * ahead; py[:, i] = x[row_y, i] + 0.01 * ahead ** 2

    def far(i):
        px[:, i] = x[row_x, i] + 1e8 + 5.0 * ahead; py[:, i] = x[row_y, i] + 1e8

    return [("ptsx[2] = nan", lambda i: px.__setitem__((2, i), np.nan)),
            ("ptsy[3] = inf", lambda i: py.__setitem__((3, i), np.inf)),
            ("all waypoints at the car", at_the_car),
            ("all waypoints at one x", one_x),
            ("waypoints behind the car, decreasing x", behind),
            ("waypoints 1e8 m away", far)]


def _model_defects(model):
    if model is None:
        return []
    return [("Lf = 0", lambda i: model.__setitem__((MODEL_LF, i), 0.0)),
            ("Lf = nan", lambda i: model.__setitem__((MODEL_LF, i), np.nan)),
            ("max_steering = 0", lambda i: model.__setitem__((MODEL_MAX_STEERING, i), 0.0))]


def _apply(defects):
    for i, (_, fn) in enumerate(defects):
        fn(i)
    return [d[0] for d in defects]


def garbage_telemetry(tel, ptsx, ptsy, model=None):
    """Copies of (tel, ptsx, ptsy, model) whose first instances carry inputs no simulator sends, one defect per instance, shaped like
    helpers.garbage_batch.  Returns (tel, ptsx, ptsy, model, names).  Every instance is owed a status other than SUCCESS, but for the
    names is_defect() refuses (WELL_POSED below)."""
    t, px, py = _f(tel), _f(ptsx), _f(ptsy)
    m = _f(model) if model is not None else None
    set_t = lambda row, v: (lambda i: t.__setitem__((row, i), v))
    defects = [("psi = " + name, set_t(2, v)) for name, v in PSI_OUT_OF_RANGE]
    defects += [("psi in range: " + name, set_t(2, v)) for name, v in PSI_IN_RANGE]
    defects += [("x = nan", set_t(0, np.nan)), ("x = inf", set_t(0, np.inf)), ("x = 1e300", set_t(0, 1e300)),
                ("y = nan", set_t(1, np.nan)), ("y = inf", set_t(1, np.inf)), ("y = 1e300", set_t(1, 1e300)),
                ("speed = nan", set_t(3, np.nan)), ("speed = inf", set_t(3, np.inf)), ("speed = -50", set_t(3, -50.0)), ("speed = 1e6", set_t(3, 1e6)),
                ("steering_angle = nan", set_t(4, np.nan)), ("steering_angle = 1e6", set_t(4, 1e6)),
                ("throttle = nan", set_t(5, np.nan)), ("throttle = inf", set_t(5, np.inf))]
    defects += _waypoint_defects(t, px, py, 0, 1, 2, at_rest=lambda i: t.__setitem__((3, i), 0.0), straight=lambda i: t.__setitem__((4, i), 0.0))
    defects += _model_defects(m)
    return t, px, py, m, _apply(defects)


def garbage_pose(pose, ptsx, ptsy, model=None):
    """The same for mpc_run_batch_*, which takes the pose itself: psi goes to the frame change as it is (no normalisation), so only the
    values outside fsincos' range are defects; v is in m/s."""
    p, px, py = _f(pose), _f(ptsx), _f(ptsy)
    m = _f(model) if model is not None else None
    set_p = lambda row, v: (lambda i: p.__setitem__((row, i), v))
    defects = [("psi = " + name, set_p(2, v)) for name, v in PSI_OUT_OF_RANGE]
    defects += [("x = nan", set_p(0, np.nan)), ("x = inf", set_p(0, np.inf)), ("x = 1e300", set_p(0, 1e300)),
                ("y = nan", set_p(1, np.nan)), ("y = inf", set_p(1, np.inf)), ("y = 1e300", set_p(1, 1e300)),
                ("v = nan", set_p(3, np.nan)), ("v = inf", set_p(3, np.inf)), ("v = 1e6", set_p(3, 1e6)),
                ("steering = nan", set_p(4, np.nan)), ("steering = 1e6", set_p(4, 1e6))]
    defects += _waypoint_defects(p, px, py, 0, 1, 2, at_rest=lambda i: None, straight=lambda i: None)
    defects += _model_defects(m)
    return p, px, py, m, _apply(defects)


# In the lists, but owed no status -- unusual and well-posed, like "v0 = -5" and "all weights 0" of helpers.garbage_batch: the psi values
# the header allows, and waypoints behind the car, which the reference provides for (the dir < 0 branch of RoadGeometry::orientation) and
# whose fit tests/golden/fit_edges.json answers exactly.  What they are owed: an end, a status code, and no effect on their neighbours.
WELL_POSED = ("psi in range", "waypoints behind the car")


def is_defect(name):
    return not name.startswith(WELL_POSED)


def population(pkg, params, waypoints, B):
    """B lake-track cars (seed 83): pose, the telemetry rows of the same cars, waypoints, and a model array of the handle's values"""
    from run_model_helpers import uniform_model
    sc = pkg.scenarios.lake_track_batch(B, params, waypoints, seed=SEED)
    pose, px, py = _f(sc["pose"]), _f(sc["ptsx"]), _f(sc["ptsy"])
    tel = _f(np.stack([pose[0], pose[1], pose[2], pose[3] * 3600.0 / 1609.34, -pose[4], np.full(B, 0.3)]))
    return {"pose": pose, "tel": tel, "ptsx": px, "ptsy": py, "model": uniform_model(params, B)}


def same_status(a, b):
    """the rule of test_garbage_inputs_get_a_status_and_stay_contained: not-a-number and overflow end in either of the two "could
    not" codes (2, 4), depending on which operation sees them first"""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isin(a, (2, 4)) & np.isin(b, (2, 4)))


# ---- the child process -----------------------------------------------------------------------------------------------------------
def _twin_run(twin, pkg, params, x, ptsx, ptsy, model, tel, warm=None, warm_status=None):
    from run_model_helpers import twin_run_model
    opts = pkg.warm_opts_default()
    B = x.shape[1]
    if model is not None:
        return twin_run_model(twin, params, x, ptsx, ptsy, model, opts, warm=warm, warm_status=warm_status, tel=tel, extra=EXTRA_LATENCY if tel else 0.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    x, px, py = _f(x), _f(ptsx), _f(ptsy)
    npts = px.shape[0]
    rows = (params.N - 1) * 22
    r = {"out8": np.zeros((8, B)), "cmd": np.zeros((2, B)), "pre": np.zeros((15, B)), "status": np.zeros(B, dtype=np.int32),
         "iters": np.zeros(B, dtype=np.int32), "warm": np.zeros((rows, B)), "ptsx": px, "ptsy": py}
    ws = np.ascontiguousarray(warm_status, dtype=np.int32) if warm_status is not None else None
    w = _f(warm) if warm is not None else None
    rc = twin.mpc_twin_run(C.byref(params), C.c_int64(B), C.c_int64(B), C.c_int(npts), vp(x), C.c_int(1 if tel else 0),
                           C.c_double(EXTRA_LATENCY if tel else 0.0), vp(px), vp(py), None, vp(w), vp(ws), vp(r["warm"]), C.c_int64(B),
                           C.byref(opts), vp(r["out8"]), vp(r["cmd"]), vp(r["status"]), vp(r["iters"]), vp(r["pre"]))
    assert rc == 0
    return r


def child_main(path):
    """Runs in the child: the clean and the dirty batch of every form through the CPU build, results into an .npz.  Calls neither the
    oracle nor anything else that may still loop on such input."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    from helpers import load_twin
    pkg = G.load_package()
    twin = load_twin()
    spec = json.load(open(path + ".json"))
    params = pkg.params_from_json(os.path.join(ROOT, "tests", "golden", spec["config"]))
    wp = pkg.scenarios.load_waypoints(os.path.join(ROOT, "tests", "golden", "lake_track_waypoints.csv"))
    pop = population(pkg, params, wp, spec["B"])
    out = {}
    with np.errstate(all="ignore"):
        for form in spec["forms"]:
            tel = form.startswith("tel")
            model = pop["model"] if form.endswith("_model") else None
            x = pop["tel"] if tel else pop["pose"]
            gx, gpx, gpy, gm, names = (garbage_telemetry if tel else garbage_pose)(x, pop["ptsx"], pop["ptsy"], model)
            clean = _twin_run(twin, pkg, params, x, pop["ptsx"], pop["ptsy"], model, tel)
            dirty = _twin_run(twin, pkg, params, gx, gpx, gpy, gm, tel)
            # warm: both batches once more, started from the clean call's records
            wclean = _twin_run(twin, pkg, params, x, pop["ptsx"], pop["ptsy"], model, tel, warm=clean["warm"], warm_status=clean["status"])
            wdirty = _twin_run(twin, pkg, params, gx, gpx, gpy, gm, tel, warm=clean["warm"], warm_status=clean["status"])
            for tag, r in (("clean", clean), ("dirty", dirty), ("wclean", wclean), ("wdirty", wdirty)):
                for k in ("out8", "cmd", "status", "iters", "pre", "ptsx", "ptsy", "warm"):
                    out["%s/%s/%s" % (form, tag, k)] = r[k]
    np.savez(path, **out)


def run_forms_in_child(forms, B, config=CONFIG, timeout=CHILD_TIMEOUT_S):
    """-> {form: {tag: {array name: array}}}; a child that does not end within `timeout` seconds fails the caller
    (subprocess.TimeoutExpired) after it has been killed"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "garbage.npz")
        json.dump({"forms": list(forms), "B": int(B), "config": config}, open(path + ".json", "w"))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=timeout, env=env)
        assert p.returncode == 0, p.stderr[-4000:]
        z = np.load(path)
        res = {}
        for key in z.files:
            form, tag, k = key.split("/")
            res.setdefault(form, {}).setdefault(tag, {})[k] = z[key]
    return res


def names_of(form, pop):
    tel = form.startswith("tel")
    model = pop["model"] if form.endswith("_model") else None
    return (garbage_telemetry if tel else garbage_pose)(pop["tel"] if tel else pop["pose"], pop["ptsx"], pop["ptsy"], model)[4]


if __name__ == "__main__":
    child_main(sys.argv[1])
