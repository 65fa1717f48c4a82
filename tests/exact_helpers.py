"""Helpers of the exact-minimiser tests (test infrastructure): the fixture tests/golden/exact_minimisers.npz (written by
tests/golden/make_exact_minimisers.py: the minimisers of the NLP to 30 digits, found in 70-digit arithmetic without a derivative
formula), its cases grouped into one batch per handle, the ONE assertion every solve path is held to, the CPU-twin paths, and the
records of the certificate tests.  Needs numpy and the fixture only.  Shared by tests/test_exact_minimisers.py and
tests/test_exact_minimisers_gpu.py."""
import json
import os

import numpy as np

from helpers import ROOT, TOL_ACCEL, TOL_COST_REL, TOL_STEER, TOL_TRAJ

QUANT = ("steer", "accel", "state", "traj", "cost")
TOL_FALLBACK = {"steer": TOL_STEER, "accel": TOL_ACCEL, "state": TOL_TRAJ, "traj": TOL_TRAJ, "cost": TOL_COST_REL}
NMAX = 25
WARM_REC = 22
MEASURED = {}          # path -> class -> quantity -> measured maximum: what profiles/exact_minimisers.json holds
_fx = None


class Fixture:
    def __init__(self, path):
        z = np.load(path)
        self.a = {k: z[k] for k in z.files if k != "meta"}
        self.meta = json.loads(str(z["meta"]))
        self.classes, self.configs, self.names = self.meta["classes"], self.meta["configs"], self.meta["names"]
        self.yard = self.meta["yardsticks"]
        self.n = len(self.names)

    def of_class(self, cls):
        return np.nonzero(self.a["cls"] == self.classes.index(cls))[0]

    def groups(self, cls, N=None):
        """The cases of a class, one group per handle (config file, N, dt), in the fixture's order: [dict(cls, config, N, dt, max_speed, idx,
        batch, weights, model, horizon)]; weights / model / horizon are None where the class has none."""
        a, out = self.a, []
        idx = self.of_class(cls)
        key = lambda i: (int(a["config"][i]), int(a["N"][i]), float(a["dt"][i]), float(np.nan_to_num(a["max_speed"][i])))
        for cfg, n, dt, vmax in sorted(set(key(i) for i in idx)):
            if N is not None and n != N:
                continue
            sel = np.array([i for i in idx if key(i) == (cfg, n, dt, vmax)])
            c = lambda v: np.ascontiguousarray(v)
            g = {"cls": cls, "config": self.configs[cfg], "N": n, "dt": dt, "max_speed": vmax or None, "idx": sel,
                 "batch": {"state": c(a["state"][:, sel]), "coeffs": c(a["coef"][:, sel]), "yaw_lo": c(a["yaw"][0, sel]), "yaw_hi": c(a["yaw"][1, sel])},
                 "weights": c(a["weights"][:, sel]) if np.isfinite(a["weights"][:, sel]).all() else None,
                 "model": c(a["model"][:, sel]) if np.isfinite(a["model"][:, sel]).all() else None,
                 "horizon": c(a["horizon"][sel].astype(np.int32)) if (a["horizon"][sel] > 0).all() else None}
            assert g["weights"] is not None or np.isnan(a["weights"][:, sel]).all()
            assert g["model"] is not None or np.isnan(a["model"][:, sel]).all()
            assert g["horizon"] is not None or (a["horizon"][sel] == 0).all()
            out.append(g)
        return out


def fixture():
    global _fx
    if _fx is None:
        _fx = Fixture(os.path.join(ROOT, "tests", "golden", "exact_minimisers.npz"))
    return _fx


def group_params(pkg, g, **over):
    """the parameter set of a group's handle: its config file at the group's N and dt (and the test's own overrides)"""
    if g["max_speed"] is not None:         # a max_speed set after the load: the speed tables keep the file's cap
        over = dict(over, max_speed=g["max_speed"])
    return pkg.params_from_json(os.path.join(ROOT, "tests", "golden", g["config"]), N=g["N"], dt=g["dt"], **over)


def reorder(g, order):
    """the same group with its instances in another order"""
    o = np.asarray(order)
    pick = lambda v: None if v is None else np.ascontiguousarray(v[..., o])
    return dict(g, idx=g["idx"][o], batch={k: pick(v) for k, v in g["batch"].items()}, weights=pick(g["weights"]), model=pick(g["model"]),
                horizon=pick(g["horizon"]))


def distances(g, got):
    """per instance and quantity: |got - exact| (the cost relative to max(1, |exact|)) -> {quantity: [n]}"""
    a = fixture().a
    idx, N = g["idx"], g["N"]
    ex = a["out"][:, idx]
    out = np.asarray(got["out"], dtype=np.float64)
    d = {"steer": np.abs(out[6] - ex[6]), "accel": np.abs(out[7] - ex[7]), "state": np.abs(out[:6] - ex[:6]).max(0),
         "cost": np.abs(out[8] - ex[8]) / np.maximum(1.0, np.abs(ex[8]))}
    if got.get("traj") is not None:
        t = np.zeros(len(idx))
        for j, i in enumerate(idx):
            n = int(a["horizon"][i]) or N
            gx, gy = got["traj"][:n, j], got["traj"][N:N + n, j]
            t[j] = max(np.abs(gx - a["traj"][:n, i]).max(), np.abs(gy - a["traj"][NMAX:NMAX + n, i]).max())
        d["traj"] = t
    return d


def assert_exact(g, got, path, fallback=False):
    """THE assertion of these tests, for every path: every case's status is SUCCESS and every quantity lies within the class
    yardstick of the exact value (fallback: within today's TOL_* of tests/helpers.py instead -- for a path whose stopping rule
    ends elsewhere, named in the test that passes it).  Prints the measured maximum beside the yardstick and keeps it in MEASURED."""
    fx = fixture()
    cls = g["cls"]
    status = np.asarray(got["status"])
    assert status.shape == (len(g["idx"]),) and (status == 0).all(), (path, cls, "status", status.tolist())
    assert np.isfinite(got["out"]).all(), (path, cls)
    d = distances(g, got)
    bad = []
    for q in QUANT:
        if q not in d:
            continue
        yard = TOL_FALLBACK[q] if fallback else fx.yard[cls][q]
        worst = float(d[q].max())
        slot = MEASURED.setdefault(path, {}).setdefault(cls, {})
        slot[q] = max(slot.get(q, 0.0), worst)
        print("%-28s %-14s N=%-2d %-6s max %.3e  yardstick %.3e%s" % (path, cls, g["N"], q, worst, yard, "  EXCEEDED at %s" % fx.names[g["idx"][int(d[q].argmax())]] if worst > yard else ""))
        if worst > yard:
            bad.append((q, worst, yard, fx.names[g["idx"][int(d[q].argmax())]]))
    assert not bad, (path, cls, bad)


# ---- the CPU twin, one function per path -----------------------------------------------------------------------------------------
def twin_paths(pkg):
    """{path name: function() that runs the CPU twin on every group of the classes the path serves and asserts}"""
    from helpers import load_twin, twin_solve, twin_solve_mixed_f64
    from horizon_helpers import load_horizon_twin, twin_horizon_solve, twin_plain_solve
    from model_helpers import twin_model_solve
    fx = fixture()

    def plain(classes, path, solve=twin_solve, **over):
        def run():
            for cls in classes:
                for g in fx.groups(cls):
                    assert_exact(g, solve(load_twin(), group_params(pkg, g, **over), g["batch"], weights=g["weights"]), path)
        return run

    def horizons_f32_start():
        for g in fx.groups("horizons", N=25):
            assert_exact(g, twin_solve_mixed_f64(load_twin(), group_params(pkg, g, f64_f32_start=1), g["batch"]), "twin f64_f32_start")

    def model():
        for g in fx.groups("model"):
            assert_exact(g, twin_model_solve(load_twin(), group_params(pkg, g), g["batch"], g["model"]), "twin _model")

    def mixed():
        for g in fx.groups("mixed_horizon"):
            for tag, gg in (("fixture order", g), ("sorted", reorder(g, np.argsort(g["horizon"], kind="stable")))):
                r = twin_horizon_solve(load_horizon_twin(), group_params(pkg, gg), gg["batch"], gg["horizon"], model=gg["model"])
                assert_exact(gg, r, "twin _horizon, " + tag)

    def warm(cls, path, use_model):
        def run():
            opts = pkg.warm_opts_default(shift=0)
            for g in fx.groups(cls):
                p = group_params(pkg, g, f64_f32_start=0)
                md = g["model"] if use_model else None
                cold = twin_plain_solve(load_twin(), p, g["batch"], opts, model=md, want_warm=True)
                assert_exact(g, cold, path + ", cold")
                again = twin_plain_solve(load_twin(), p, g["batch"], opts, model=md, warm=cold["warm"], warm_status=cold["status"])
                assert_exact(g, again, path + ", warm")
        return run
    return {"twin plain": plain(("plain", "a_free"), "twin plain"), "twin weights": plain(("weights",), "twin weights"),
            "twin horizons": plain(("horizons",), "twin horizons", f64_f32_start=0), "twin f64_f32_start": horizons_f32_start,
            "twin _model": model, "twin _horizon": mixed, "twin _warm": warm("plain", "twin _warm", False),
            "twin _warm_model": warm("model", "twin _warm_model", True)}


# ---- the certificate at exact points -----------------------------------------------------------------------------------------------
def record_groups():
    """The 24 stored records, one group per handle like Fixture.groups: [dict(... , sol [2][(N-1) * 22, n]: the exact points and their
    perturbed copies, rows [2][12, n], sizes [2][5, n] (X, Lam, df, sd, sc), verdict [2][n])]"""
    fx = fixture()
    a = fx.a
    out = []
    for cls in fx.classes:
        for g in fx.groups(cls):
            pos = [int(np.nonzero(a["rec_case"] == i)[0][0]) for i in g["idx"] if i in a["rec_case"]]
            if not pos:
                continue
            keep = np.array([j for j, i in enumerate(g["idx"]) if i in a["rec_case"]])
            gg = reorder(g, keep)
            rows = (g["N"] - 1) * WARM_REC
            gg["sol"] = [np.ascontiguousarray(a["rec"][v][:rows, pos]) for v in (0, 1)]
            assert np.isfinite(gg["sol"][0]).all() and np.isfinite(gg["sol"][1]).all()
            gg["rows"] = [a["rec_rows"][v][:, pos] for v in (0, 1)]
            gg["sizes"] = [a["rec_sizes"][v][:, pos] for v in (0, 1)]
            gg["verdict"] = [a["rec_verdict"][v][pos] for v in (0, 1)]
            out.append(gg)
    assert sum(len(g["idx"]) for g in out) == len(a["rec_case"]) == 24
    return out


def assert_certificates(g, certify, what):
    """certify(sol) -> {"cert" [12, >= n], "verdict"}: the code under test on the group's exact records and on their perturbed copies,
    row by row against the fixture's rows with the rounding bounds certify_helpers.assert_rows states, and the verdict the header's
    rule gives on the exact rows."""
    from certify_helpers import BOUND_VIOL, NOT_A_POINT, assert_rows
    n = len(g["idx"])
    for v, tag in enumerate(("exact", "perturbed")):
        got = certify(g["sol"][v])
        for j in range(n):
            name = (what, tag, fixture().names[g["idx"][j]])
            want = int(g["verdict"][v][j])
            assert int(got["verdict"][j]) == want, (name, int(got["verdict"][j]), want, got["cert"][:, j].tolist())
            if want == NOT_A_POINT:
                assert abs(got["cert"][BOUND_VIOL, j] - g["rows"][v][BOUND_VIOL, j]) <= 1e-15, name
                continue
            X, Lam, df, sd, sc = g["sizes"][v][:, j]
            assert_rows(got["cert"][:, j], {"rows": g["rows"][v][:, j], "X": X, "Lam": Lam, "df": df, "sd": sd, "sc": sc}, name)
