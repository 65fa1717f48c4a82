"""Conformance of the solver's own math (csrc/mpc_core.h: fsincos2, frcp, frcp1, fatan, flog, hpow; fp64 and fp32) against the exact
answers of tests/golden/math_edges.npz (mpmath at 120 digits, tests/golden/make_math_edges.py), on the device (mpc_debug_math_all) and
in the CPU twin (mpc_host_twin_math_all): the same fixture, the same bounds, one assertion helper.  One call per build evaluates every
point of every function; no solve runs.

Bounds (errors against the exact answer; "rel" is |error| / |exact|, and an exact 0 must be returned as 0):
  f64 sincos   abs 4e-16 for |x| < 1e9, each of sin x, cos x, sin y, cos y; rel 4e-16 where |exact| >= 1e-6 (the two-part Cody-Waite
               reduction leaves at most k * 7e-33 <= 4.5e-24 absolute)
  f64 frcp     rel 2^-53 (1 + 2^-20), normal x with normal 1/x: seed 4.6e-8 -> e^2 -> e^4 ~ 4e-30, then one rounding
  f64 frcp1    rel 2.5e-15: (4.6e-8)^2 + 2^-53 = 2.23e-15, plus 10 %
  f64 fatan    rel 4.1e-16 (the statement of mpc_core.h)
  f64 flog     rel 2.3e-16 for every positive finite x, subnormals included, with no floor near 1 ("< 1 ulp")
  hpow         rel 2^-21 max(1, |p log2 x|) where x^p is a normal float, both types.  On the device x^p = exp2f(pf * log2f((float)x)):
               with t = p log2 x, the error of t is |t| (2^-23 [log2f, 1 ulp] + 2^-24 [the product] + 2^-25.4 [p as a float]) plus
               2^-24 / ln 2 * p [x as a float], and d(2^t)/2^t = ln 2 dt, plus 2^-23 [exp2f, 1 ulp]:
               0.29 |t| 2^-21 + 0.54 2^-21 <= 0.83 * 2^-21 max(1, |t|)
  f32 sincos   abs 1.5e-7 for |x| < 1e4: the stated approximation error 8e-8 plus half an ulp of 1
  f32 fatan    abs 7e-8 for |x| <= 1 (stated), abs 2.5e-7 for |x| > 1 (derived: 2.3e-7)
  f32 frcp(1)  rel 2^-23, normal x with normal 1/x ("1 ulp")
  f32 flog     rel 2^-22, normal x: 1 ulp of log2, the rounding of the multiplication, the constant

WHERE THE TWO BUILDS LEGITIMATELY DIFFER (everything else below is asserted alike for both; `edge_*` pin each line):
  argument                         device                                   CPU twin                 why no caller depends on it
  frcp, frcp1 (f64): 0, +-inf      NaN: fma(-0, inf, 1), fma(-inf, 0, 1)    +-inf, +-0 (1.0 / x)     a slack or pivot of 0 or inf has
  frcp, frcp1 (f64): 1/x overflows NaN (the seed is inf)                    +-inf                    cleared Ev.ok / failed the pivot test
  frcp, frcp1 (f64): 1/x subnormal 1/x to two steps of 2^-1074             1.0 / x                  before its reciprocal is used
  frcp, frcp1 (f32): subnormal x   +-inf (v_rcp_f32 flushes its argument)   1.0f / x                 fp32 slacks: see edge_flog
  frcp, frcp1 (f32): 1/x subnormal +-0 (v_rcp_f32 flushes its result)       1.0f / x                 (the same)
  fatan: +-inf                     f64 NaN (frcp(inf)); f32 +-pi/2          +-pi/2                   a slope of inf has no fit
  flog (f32): subnormal x          -inf (v_log_f32 flushes its argument)    logf(x)                  see edge_flog
  hpow: x > 1e16                   hpow(1e16) (the clamp)                   pow(x, p), unclamped     thresholds of the switching
  hpow: x^p below the floats       0 or a float subnormal                   pow(x, p)                condition, compared, never stored
  hpow: NaN                        hpow(1e16): fmin(NaN, 1e16) = 1e16       NaN                      a NaN theta has cleared Ev.ok
  hpow: -inf                       NaN                                      +inf (C's pow)           theta >= 0, -dphi > 0 at the call
The same in both builds: flog (f64) of 0 is the FINITE -4.7507 (f = -1, s = -1 go through the kernel), of a negative or inf NaN; flog
(f32) of 0 is -inf, of a negative NaN; hpow of a negative finite is NaN.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FUNCS = [p + f for p in ("f64_", "f32_") for f in ("sincos", "frcp", "frcp1", "fatan", "flog", "hpow")]
ROWS = {"sincos": (0, 1, 2, 3), "frcp": (4,), "frcp1": (5,), "fatan": (6,), "flog": (7,), "hpow": (8, 9)}
NROWS = 20
MIRROR = {"sincos": (-1.0, 1.0), "frcp": (-1.0,), "frcp1": (-1.0,), "fatan": (-1.0,)}   # answer(-x) = sign * answer(x), per row of F.hi
SHIFT = 7                    # slot b of fsincos2 gets the point list rotated by this many places: x != y in every pair
PARTNERS = (3, 50, 333)      # the valid points an out-of-range sincos argument is paired with
S_THETA, S_PHI = 1.1, 2.3
TINY32 = float(np.finfo(np.float32).tiny)


class Layout:
    """Every function's points in one pair of argument arrays, and where they are."""

    def __init__(self):
        z = np.load(os.path.join(HERE, "golden", "math_edges.npz"))
        self.x, self.hi, self.lo, self.edge, self.at, self.edge_at = {}, {}, {}, {}, {}, {}
        xs, ys, n = [], [], 0
        for name in FUNCS:
            x = z[name + ".x"].astype(np.float64); hi = z[name + ".hi"]; lo = z[name + ".lo"].astype(np.float64)
            edge = z[name + ".edge"].astype(np.float64)
            sign = MIRROR.get(name[4:])
            if sign is not None:
                assert (x >= 0).all()
                s = np.array(sign)[:, None]
                x = np.concatenate([x, -x]); hi = np.concatenate([hi, s * hi], axis=1); lo = np.concatenate([lo, s * lo], axis=1)
            self.x[name], self.hi[name], self.lo[name], self.edge[name] = x, hi, lo, edge
            if name.endswith("sincos"):
                # main pairs (x_i, x_{i - SHIFT}); then (valid, out of range) and (out of range, valid) for every edge value
                va = np.repeat(x[list(PARTNERS)], len(edge)); ed = np.tile(edge, len(PARTNERS))
                ax = np.concatenate([x, va, ed]); ay = np.concatenate([np.roll(x, SHIFT), ed, va])
            else:
                ax = np.concatenate([x, edge]); ay = ax
            self.at[name] = slice(n, n + len(x)); self.edge_at[name] = slice(n + len(x), n + len(ax))
            xs.append(ax); ys.append(ay); n += len(ax)
        self.ax = np.ascontiguousarray(np.concatenate(xs)); self.ay = np.ascontiguousarray(np.concatenate(ys))
        self.n = n

    def rows(self, name):
        return [r + (10 if name.startswith("f32") else 0) for r in ROWS[name[4:]]]

    def got(self, out, name):
        """[rows][points of the function], [rows][its edge arguments]"""
        r = self.rows(name)
        return out[r][:, self.at[name]], out[r][:, self.edge_at[name]]

    def errors(self, out, name):
        """the error of every result against the exact answer, [rows][points]; NaN where the fixture has no answer (hpow)"""
        got, _ = self.got(out, name)
        hi, lo = self.hi[name], self.lo[name]
        if name.endswith("sincos"):            # slot b holds the same points SHIFT places on
            hi = np.concatenate([hi, np.roll(hi, SHIFT, axis=1)]); lo = np.concatenate([lo, np.roll(lo, SHIFT, axis=1)])
        with np.errstate(invalid="ignore"):
            return (got - hi) - lo * np.spacing(np.abs(hi)), hi


@pytest.fixture(scope="module")
def layout():
    return Layout()


def evaluate_twin(twin, L):
    out = np.zeros((NROWS, L.n))
    twin.mpc_host_twin_math_all.argtypes = [C.c_int64] + [C.c_void_p] * 3
    assert twin.mpc_host_twin_math_all(L.n, L.ax.ctypes.data, L.ay.ctypes.data, out.ctypes.data) == 0
    return out


def evaluate_device(pkg, L):
    from carnd_mpc_project_amd._abi import check
    out = np.zeros((NROWS, L.n))
    check(pkg.library().mpc_debug_math_all(0, L.n, L.ax.ctypes.data, L.ay.ctypes.data, out.ctypes.data), "mpc_debug_math_all")
    return out


@pytest.fixture(scope="module")
def twin_out(host_twin, layout):
    return evaluate_twin(host_twin, layout)


@pytest.fixture(scope="module")
def device_out(pkg, layout):
    return evaluate_device(pkg, layout)


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def rel(err, ref):
    """|err| / |ref|; an exact 0 must be returned as 0 (inf otherwise)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref == 0, np.where(err == 0, 0.0, np.inf), np.abs(err) / np.abs(ref))


def measure(L, out, name):
    """-> [(what, measured maximum, bound)] of one function: every point of its list is in at least one line"""
    err, ref = L.errors(out, name)
    x = L.x[name]
    f32 = name.startswith("f32")
    kind = name[4:]
    if kind == "sincos":
        res = []
        for r, what in enumerate(("sin x", "cos x", "sin y", "cos y")):
            res.append(("abs %s" % what, np.max(np.abs(err[r])), 1.5e-7 if f32 else 4e-16))
            if not f32:
                m = np.abs(ref[r]) >= 1e-6
                res.append(("rel %s, |exact| >= 1e-6" % what, np.max(rel(err[r], ref[r])[m]), 4e-16))
        return res
    if kind in ("frcp", "frcp1"):
        bound = 2.0 ** -23 if f32 else (2.0 ** -53 * (1 + 2.0 ** -20) if kind == "frcp" else 2.5e-15)
        return [("rel", np.max(rel(err[0], ref[0])), bound)]
    if kind == "fatan":
        if f32:
            m = np.abs(x) <= 1
            return [("abs, |x| <= 1", np.max(np.abs(err[0][m])), 7e-8), ("abs, |x| > 1", np.max(np.abs(err[0][~m])), 2.5e-7)]
        return [("rel", np.max(rel(err[0], ref[0])), 4.1e-16)]
    if kind == "flog":
        return [("rel", np.max(rel(err[0], ref[0])), 2.0 ** -22 if f32 else 2.3e-16)]
    res = []
    for r, p in enumerate((S_THETA, S_PHI)):
        m = np.isfinite(ref[r])
        assert m.sum() > 100
        scale = np.maximum(1.0, np.abs(p * np.log2(x[m])))
        res.append(("rel / max(1, |p log2 x|), p = %g" % p, np.max(rel(err[r][m], ref[r][m]) / scale), 2.0 ** -21))
    return res


def assert_bounds(L, out, name, build):
    res = measure(L, out, name)
    for what, got, bound in res:
        print("%-6s %-10s %-36s %.4g (bound %.4g)" % (build, name, what, got, bound))
    bad = [(what, got, bound) for what, got, bound in res if not got <= bound]
    assert not bad, (build, name, bad)


# ---- the arguments no caller should send --------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def edge_sincos(L, out, name, build):
    """Beyond the reduction's range (|x| >= 1e9 / 1e4, inf, NaN) the slot is NaN -- the solver flags the evaluation and rejects the trial
    step -- and ONLY that slot: the other slot's sine and cosine are bit for bit what the same argument gave beside a valid one."""
    got, eg = L.got(out, name)
    ne, n = len(L.edge[name]), len(L.x[name])
    half = ne * len(PARTNERS)
    for j, p in enumerate(PARTNERS):
        a = slice(j * ne, (j + 1) * ne); b = slice(half + j * ne, half + (j + 1) * ne)
        assert np.isnan(eg[2:, a]).all() and np.isnan(eg[:2, b]).all(), (build, name)                  # the slot out of range
        for r in (0, 1):
            assert bits_equal(eg[r, a], np.full(ne, got[r, p])), (build, name, "slot a beside an invalid slot b")
            assert bits_equal(eg[2 + r, b], np.full(ne, got[2 + r, (p + SHIFT) % n])), (build, name, "slot b beside an invalid slot a")
        assert np.isfinite(got[:2, p]).all() and np.isfinite(got[2:, (p + SHIFT) % n]).all()


def edge_rcp(L, out, name, build):
    """The twin divides (IEEE).  The device's Newton steps turn a seed of inf or 0 into NaN: fma(-0, inf, 1), fma(-inf, 0, 1) -- every
    call site that can see such a slack or pivot has cleared Ev.ok (`!(sl > 0)`) or failed the pivot test before the value is used, and
    a NaN there keeps it cleared.  fp32 on the device is the raw v_rcp_f32, which follows IEEE at 0 and inf and flushes subnormals (its
    argument to 0, so 1/x = inf; its result to 0) although the kernels keep fp32 subnormals elsewhere -- measured on gfx950 and pinned
    (the fp32 solver's slacks do not get there: edge_flog)."""
    _, eg = L.got(out, name)
    e = L.edge[name]
    f32 = name.startswith("f32")
    dt = np.float32 if f32 else np.float64
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        ieee = (dt(1) / e.astype(dt)).astype(np.float64)
    eg = eg[0]
    if build == "twin":
        nan = np.isnan(e)
        assert np.isnan(eg[nan]).all() and bits_equal(eg[~nan], ieee[~nan]), (name, e, eg, ieee)     # (a NaN's payload is not pinned)
        return
    tiny = float(np.finfo(dt).tiny)
    for x, g, want in zip(e, eg, ieee):
        if np.isnan(x):
            assert np.isnan(g)
        elif f32:
            if x == 0 or np.isinf(x):
                assert g == want and np.signbit(g) == np.signbit(want), (name, x, g)       # +-inf, +-0 as IEEE
            else:                                                # v_rcp_f32 flushes subnormals, argument and result: +-inf, +-0
                assert g == np.copysign(np.inf if abs(x) < tiny else 0.0, x) and np.signbit(g) == np.signbit(x), (name, x, g)
        elif x == 0 or np.isinf(x) or np.isinf(want):
            assert np.isnan(g), (name, x, g)                                                # 0, inf, 1/x overflows: NaN
        elif abs(want) < tiny:
            assert abs(g - want) <= 2 * 2.0 ** -1074, (name, x, g)                          # 1/x subnormal: fp64 keeps subnormals
        else:
            assert abs(g - want) <= 2.5e-15 * abs(want), (name, x, g)                       # largest subnormal x: 1/x is normal


def edge_fatan(L, out, name, build):
    """+-inf: the fp64 device has frcp(inf) = NaN inside; everything else returns +-pi/2.  NaN stays NaN."""
    _, eg = L.got(out, name)
    e, eg = L.edge[name], eg[0]
    assert np.isinf(e[0]) and np.isinf(e[1]) and np.isnan(e[2]) and np.isnan(eg[2])
    if build == "device" and name == "f64_fatan":
        assert np.isnan(eg[:2]).all()
    else:
        assert np.allclose(eg[:2], [np.pi / 2, -np.pi / 2], rtol=2e-7 if name.startswith("f32") else 4e-16, atol=0)


def edge_flog(L, out, name, build):
    """flog's argument is a product of eight slacks, each tested `!(sl > 0) -> Ev.ok = false` before the product is taken (and a NaN
    sum clears Ev.ok afterwards), so a negative, inf or NaN reaches flog only in an evaluation that is rejected anyway: NaN or inf in
    every build.  A product of exactly 0 needs eight POSITIVE slacks to underflow together.
    fp64 (both builds): flog(0) is the finite -4.7507, a value a caller would take -- unreachable: slacks to bounds of order 0.1 .. 100
    are at least an ulp of the bound, > 1e-17, and eight of them > 1e-136, far from 1e-308.
    fp32: the eight factors are sl, su of four variables with sl + su = hi - lo, so of each pair one factor is at least half the range
    (0.1 .. 50) and only four can be small; a small one is at least an fp32 ulp of its bound, 1e-8 for a bound of 0.1: the product is
    above 1e-32 times the half ranges, far from 1.2e-38.  (A lower bound of exactly 0 has no ulp floor: that one slack would have to
    fall below 1e-14 with three others at their last ulp.)  Should it happen, the device errs to the safe side: v_log_f32 flushes a subnormal
    argument and returns -inf like for 0 (measured on gfx950, pinned), the merit function becomes +inf and the trial step is rejected;
    logf in the twin returns the logarithm.  No build returns a finite value above log(2^-126)."""
    _, eg = L.got(out, name)
    e, eg = L.edge[name], eg[0]
    f32 = name.startswith("f32")
    for x, g in zip(e, eg):
        if np.isnan(x) or x < 0:
            assert np.isnan(g) or np.isinf(g), (build, name, x, g)
        elif x == 0:
            if f32:
                assert g == -np.inf, (build, name, x, g)
            else:
                assert abs(g + 4.750706203638275) < 1e-14, (build, name, x, g)      # finite, and unreachable (above)
        elif np.isinf(x):
            assert np.isnan(g) if not f32 else g == np.inf, (build, name, x, g)
        else:                                                              # an fp32 subnormal
            assert f32 and x < TINY32
            want = np.log(x)
            if build == "twin":
                assert abs(g - want) <= 2.0 ** -22 * abs(want), (name, x, g)
            else:
                assert g == -np.inf, (name, x, g)


def edge_hpow(L, out, name, build):
    """hpow(0) = 0; beyond 1e16 the device returns hpow(1e16) (the clamp keeps (float)x finite) where the twin's pow goes on growing;
    where x^p is below the normal floats the device returns 0 or a float subnormal (the twin: pow); a negative gives NaN; NaN gives NaN in
    the twin and hpow(1e16) on the device, whose fmin drops it (theta = NaN has cleared Ev.ok, mpc_core.h "Ev.theta == Ev.theta", and
    -dphi is only passed when dphi < 0).  These are thresholds of the line search's switching condition (theta^1.1, (-dphi)^2.3),
    compared and never stored."""
    got, eg = L.got(out, name)
    e, x = L.edge[name], L.x[name]
    f32 = name.startswith("f32")
    dt = np.float32 if f32 else np.float64
    clamp = dt(1e16)
    i16 = int(np.nonzero(x == float(clamp))[0][0])
    for r, p in enumerate((float(dt(S_THETA)), float(dt(S_PHI)))):
        for xv, g in zip(e, eg[r]):
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                want = float(dt(xv) ** dt(p)) if xv >= 0 else np.nan
            if xv == -np.inf and build == "twin":
                assert g == np.inf, (build, name, xv, g)                   # C's pow(-inf, non-integer > 0)
            elif np.isnan(xv) and build == "device":
                assert g == got[r, i16], (name, xv, g)                     # fmin(NaN, 1e16) = 1e16
            elif np.isnan(xv) or xv < 0:
                assert np.isnan(g), (build, name, xv, g)
            elif xv == 0:
                assert g == 0, (build, name, xv, g)
            elif xv > float(clamp):
                if build == "device":
                    assert g == got[r, i16], (name, xv, g)
                else:
                    assert g == want or abs(g - want) <= 2.0 ** -21 * want * max(1.0, abs(p * np.log2(xv))), (name, xv, g)
            else:                                                          # (float)x subnormal or 0: x^p far below the normal floats
                assert 0 <= g <= TINY32, (build, name, xv, g)
                if build == "device" and xv < 2.0 ** -150:
                    assert g == 0, (name, xv, g)
        # the points of the list where x^p is no normal float (the lower end of each exponent): 0 or below the smallest normal float
        m = ~np.isfinite(L.hi[name][r])
        assert m.sum() >= (5 if r == 0 else 15)
        assert ((got[r][m] >= 0) & (got[r][m] <= TINY32 * (1 + 2.0 ** -20))).all(), (build, name, p, x[m], got[r][m])


EDGE = {"sincos": edge_sincos, "frcp": edge_rcp, "frcp1": edge_rcp, "fatan": edge_fatan, "flog": edge_flog, "hpow": edge_hpow}


def check_function(L, out, name, build):
    assert len(L.x[name]) > 150 and out.shape == (NROWS, L.n)
    assert_bounds(L, out, name, build)
    EDGE[name[4:]](L, out, name, build)


@pytest.mark.parametrize("name", FUNCS)
def test_twin_math_conformance(layout, twin_out, name):
    """The CPU build of mpc_core.h: the polynomial kernels, reductions and compensated forms (the same source as on the device; its
    reciprocal, fp32 log and hpow are libm's, so those lines check the fixture and the harness more than the solver)."""
    check_function(layout, twin_out, name, "twin")


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUNCS)
def test_device_math_conformance(layout, device_out, name):
    """The same on the device: v_rcp_f64 + Newton steps, v_rcp_f32, v_log_f32, exp2f(p log2f x), and the kernels as hipcc contracts
    them.  One launch of mpc_debug_math_all for all twelve functions."""
    check_function(layout, device_out, name, "device")


def maxima(L, out):
    return {name: {what: float("%.4g" % got) for what, got, _ in measure(L, out, name)} for name in FUNCS}


if __name__ == "__main__":
    # python tests/test_math_conformance.py [--device]: the measured maxima of profiles/math_conformance.json, as JSON
    sys.path.insert(0, os.path.dirname(HERE))
    L = Layout()
    if "--device" in sys.argv[1:]:
        import __graft_entry__ as G
        print(json.dumps({"device": maxima(L, evaluate_device(G.load_package(), L))}, indent=1))
    else:
        print(json.dumps({"twin": maxima(L, evaluate_twin(C.CDLL(os.path.join(HERE, "host_twin", "libhost_twin.so")), L))}, indent=1))
