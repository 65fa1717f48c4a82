"""Generator of tests/golden/fit_edges.json: the adaptive polynomial fit of run() (RoadGeometry::fit, csrc/mpc_run_core.h) at its edges,
answered EXACTLY -- the waypoints are taken as the rationals their doubles are and the least squares problems are solved with mpmath
at 120 digits -- plus the exact reductions of the psi values of tests/run_garbage_helpers.py.

    python tests/golden/make_fit_edges.py          (needs mpmath; the oracle library is built on the way)

Cases (every one with vehicle-frame waypoints: the tests hand them over with the pose (0, 0, 0), which leaves them as they are):
  forced     every npts 3..8 x final order 2, 3, 4 (max_fit_error = 0, max_fit_order = 3, 4, 5) on: spacings 1e-3 .. 50 m, x offsets 30 and
             1e3 m (ill-conditioned), negative x, waypoints behind the car in decreasing x, irregular, clustered and repeated x
  natural    max_fit_order = 5, max_fit_error = NATURAL_ERROR: y scaled so that the exact residual of order 2 (of order 3) is 5 % below
             or 5 % above the threshold -- a margin no correct implementation loses
  degenerate all waypoints at one x, all at the car
A case is "unique" when every least squares problem on the exact path has one solution and no comparison of the exact path is an
equality; else "count_only": the residual of an interpolating fit is exactly 0, which sits ON `err > 0`, and a fit with fewer distinct
x than coefficients has many solutions -- there the fixture lists the coefficient counts a correct implementation may report.

Per unique case the fixture also holds the error of two plain references against the exact answer, numpy.linalg.lstsq on the same
Vandermonde matrix and the oracle's Householder QR (orc_polyfit): the yardstick of the tests (8 x the larger of the two, at least 4 ulp
of the quantity)."""
import ctypes as C
import json
import os
import subprocess
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
mp.mp.dps = 120
NATURAL_ERROR = 0.01
PSI_VALUES = [1e9 - 1, 200 * np.pi + 0.3, -(200 * np.pi + 0.3), 64 * np.pi, -64 * np.pi, 202.0, 202.00000000000003, -203.5, 1e3, -12345.678,
              1e6 + 0.5, -7.5e5, 3.3e8, -(1e9 - 1), 65 * np.pi, 1e9 - 64.0]


def exact_fit(x, y, ncoef):
    """-> (coefficients or None when not unique, exact squared residual)"""
    n = len(x)
    X = [mp.mpf(float(v)) for v in x]; Y = [mp.mpf(float(v)) for v in y]
    distinct = len(set(float(v) for v in x))
    if distinct >= ncoef:
        A = mp.matrix(n, ncoef)
        for i in range(n):
            for j in range(ncoef):
                A[i, j] = X[i] ** j
        c = mp.lu_solve(A.T * A, A.T * mp.matrix(Y))
        c = [c[j] for j in range(ncoef)]
        res = sum((Y[i] - sum(c[j] * X[i] ** j for j in range(ncoef))) ** 2 for i in range(n))
        if n == ncoef:
            res = mp.mpf(0)                       # interpolation: exactly zero, not the 1e-200 the digits leave
        return c, res
    # fewer distinct x than coefficients: the polynomial interpolates the mean y of every distinct x; many solutions, one residual
    groups = {}
    for xv, yv in zip(x, Y):
        groups.setdefault(float(xv), []).append(yv)
    res = sum(sum((v - sum(g) / len(g)) ** 2 for v in g) for g in groups.values())
    return None, res


def exact_path(x, y, max_fit_order, max_fit_error):
    """RoadGeometry::fit in exact arithmetic -> (ncoef, coefficients, residual of every order tried, unique?, counts allowed)"""
    order, res, unique, allowed = 2, [], True, None
    thr = mp.mpf(float(max_fit_error))
    while True:
        used = order; order += 1
        c, r = exact_fit(x, y, used + 1)
        res.append(r)
        if c is None:
            unique = False
        more = order < max_fit_order
        if more and r == thr:                     # the comparison is an equality: either way is right
            unique = False
            allowed = list(range(used + 1, max_fit_order + 1))
        if not (r > thr and more):
            break
    if allowed is None:
        allowed = [used + 1]
    return used + 1, c, res, unique, allowed


def poly_res(c, x, y):
    """the squared residual that double coefficients leave, itself exact: what is compared is the fit, not the rounding of eight
    subtractions y - f(x), which at a residual of 1e-6 on y of 2 is larger than the difference between two fits"""
    X = [mp.mpf(float(v)) for v in x]; Y = [mp.mpf(float(v)) for v in y]
    return sum((Y[i] - sum(mp.mpf(float(cj)) * X[i] ** j for j, cj in enumerate(c))) ** 2 for i in range(len(X)))


def reference_errors(x, y, ncoef, exact_c, exact_res, orc):
    """|reference - exact| for c0, c1, epsi0 = -atan(c1) and the residual: numpy.linalg.lstsq and the oracle's QR"""
    out = {}
    V = np.vander(x, ncoef, increasing=True)
    c_np = np.linalg.lstsq(V, y, rcond=None)[0]
    c_or = np.zeros(ncoef)
    DP = C.POINTER(C.c_double)
    rc = orc.orc_polyfit(x.ctypes.data_as(DP), y.ctypes.data_as(DP), len(x), ncoef - 1, c_or.ctypes.data_as(DP))
    assert rc == 0
    for name, c in (("lstsq", c_np), ("oracle", c_or)):
        out[name] = {"c0": float(abs(mp.mpf(float(c[0])) - exact_c[0])), "c1": float(abs(mp.mpf(float(c[1])) - exact_c[1])),
                     "epsi0": float(abs(mp.mpf(float(-np.arctan(c[1]))) + mp.atan(exact_c[1]))),
                     "res": float(abs(poly_res(c, x, y) - exact_res))}
    return out


def x_sets(n, rng):
    k = np.arange(n, dtype=np.float64)
    sets = [("spacing %g m" % h, h * (k + 1)) for h in (1e-3, 0.1, 5.0, 50.0)]
    sets += [("offset 30 m", 30.0 + 5.0 * k), ("offset 1e3 m", 1e3 + 5.0 * k), ("behind, decreasing x", -5.0 * (k + 1)),
             ("around the car", -12.0 + 5.0 * k), ("irregular", np.cumsum(rng.uniform(2.0, 14.0, n)) - 3.0)]
    cl = 6.0 * (k // 2 + 1) + 1e-6 * (k % 2)
    sets.append(("clustered pairs", cl))
    rp = 6.0 * (k + 1); rp[-1] = rp[-2]
    sets.append(("one x repeated", rp))
    return sets


def road(x):
    """a smooth road that is no polynomial, over the stretch of the waypoints"""
    mid, span = 0.5 * (x.max() + x.min()), max(x.max() - x.min(), 1e-9)
    u = (x - mid) / span
    return 2.0 * np.sin(1.7 * u + 0.4) + 0.8 * u ** 3 - 0.5 * np.cos(3.1 * u)


def main():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    import oracle_lib as O
    orc = O.lib()
    rng = np.random.default_rng(20240607)
    cases = []

    def add(kind, name, x, y, max_fit_order, max_fit_error):
        x = np.ascontiguousarray(x, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
        ncoef, c, res, unique, allowed = exact_path(x, y, max_fit_order, max_fit_error)
        case = {"kind": kind, "name": name, "npts": len(x), "max_fit_order": max_fit_order, "max_fit_error": max_fit_error,
                "x": x.tolist(), "y": y.tolist(), "unique": bool(unique), "ncoef": ncoef if unique else None, "ncoef_allowed": allowed,
                "res": [float(r) for r in res]}
        if unique:
            cc = [float(v) for v in c] + [0.0] * (5 - ncoef)
            case.update({"c": cc, "f0": cc[0], "epsi0": float(-mp.atan(c[1])),
                         "ref_err": reference_errors(x, y, ncoef, c, res[-1], orc)})
        cases.append(case)

    for n in range(3, 9):
        for label, x in x_sets(n, rng):
            y = road(x)
            if label == "one x repeated":
                y[-1] += 0.25
            for mfo in (3, 4, 5):
                add("forced", label, x, y, mfo, 0.0)
        # natural escalation: the exact residual of order 2 / order 3 at 0.95 and 1.05 of the threshold
        x = np.cumsum(rng.uniform(6.0, 13.0, n)) - 2.0
        g = road(x)
        for ncf in (3, 4):
            if n <= ncf:
                continue                          # interpolation: the residual is 0, nothing to place beside the threshold
            _, r = exact_fit(x, g, ncf)
            for side in (0.95, 1.05):
                s = float(mp.sqrt(mp.mpf(NATURAL_ERROR) * side / r))
                add("natural", "order %d residual at %.2f of max_fit_error" % (ncf - 1, side), x, s * g, 5, NATURAL_ERROR)
        add("degenerate", "all waypoints at one x", np.full(n, 10.0), 0.5 * np.arange(1, n + 1), 5, NATURAL_ERROR)
        add("degenerate", "all waypoints at the car", np.zeros(n), np.zeros(n), 5, NATURAL_ERROR)
    for c in cases:
        if c["kind"] == "natural":
            assert c["unique"] and min(abs(r / NATURAL_ERROR - 1.0) for r in c["res"]) > 0.04, c
    psi = []
    two_pi = 2 * mp.pi
    for v in PSI_VALUES:
        a = mp.mpf(float(v))
        r = a - two_pi * mp.floor((a + mp.pi) / two_pi)          # the exact remainder in [-pi, pi)
        psi.append({"psi": float(v), "exact": float(r), "ulp": float(np.spacing(abs(float(v))))})
    doc = {"generator": "tests/golden/make_fit_edges.py", "digits": mp.mp.dps, "natural_max_fit_error": NATURAL_ERROR,
           "cases": cases, "psi": psi}
    path = os.path.join(HERE, "fit_edges.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases (%d unique), %d psi values, %d bytes" % (len(cases), sum(c["unique"] for c in cases), len(psi), os.path.getsize(path)))


if __name__ == "__main__":
    main()
