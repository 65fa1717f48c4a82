"""Generator of tests/golden/math_edges.npz: the points at which the light-weight math of csrc/mpc_core.h (fsincos2, frcp, frcp1, fatan,
flog, hpow; fp64 and fp32) can go wrong, answered EXACTLY -- every argument is taken as the rational its double / float is and the
function is evaluated with mpmath at 120 digits.

    python tests/golden/make_math_edges.py            writes the fixture (needs mpmath)
    python tests/golden/make_math_edges.py --check    regenerates it in memory and compares byte for byte

The tests (tests/test_math_conformance.py) never import mpmath; they read, per function F of FUNCS:
  F.x    the arguments with an exact answer, as the doubles (f64_*) / floats (f32_*) they are.  The odd / even functions (sincos, frcp,
         frcp1, fatan) hold x >= 0 only: the test evaluates -x as well, whose exact answer is the mirrored one.
  F.hi   [rows][n] float64: the exact answer rounded to the nearest double (rows: sincos sin, cos; hpow exponents 1.1, 2.3; else 1).
         NaN in an hpow row: x^p is no normal float there (the bound of the test does not apply, the value is pinned separately).
  F.lo   [rows][n] float32: (exact - hi) / ulp(hi) with ulp(hi) = numpy.spacing(|hi|), in [-1/2, 1/2].  The error of a result is
         (got - hi) - lo * ulp(hi), good to 2^-24 ulp of a double.  (In units of ulp(hi), not absolute: an absolute float32
         residual underflows for |hi| < 1e-22, where frcp's half-ulp bound needs it most.)
  F.edge the arguments no caller should send (+-inf, NaN, 0, subnormals, out of range ...): no exact answer is needed for them, the test
         states what each build returns.

Points per function: see the functions below.  Random samples are seeded; the archive is written with fixed time stamps."""
import io
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "math_edges.npz")
mp.mp.dps = 120
F64, F32 = np.float64, np.float32
S_THETA, S_PHI = 1.1, 2.3                      # IpmConst::s_theta, s_phi: the only exponents hpow is called with
FUNCS = [p + f for p in ("f64_", "f32_") for f in ("sincos", "frcp", "frcp1", "fatan", "flog", "hpow")]


def nbrs(v, n, dt):
    """v and its n neighbours on either side in the format dt"""
    v = dt(v)
    out = [v]
    lo = hi = v
    for _ in range(n):
        lo = np.nextafter(lo, dt(-np.inf)); hi = np.nextafter(hi, dt(np.inf))
        out += [lo, hi]
    return out


def rnd(v, dt):
    """an mpmath value rounded to the nearest dt"""
    return dt(float(v)) if dt is F64 else F32(float(v))     # float -> float32 double-rounds: harmless for picking a test point


def uniq(points, dt, keep):
    a = np.array([p for p in points], dtype=dt)
    a = a[keep(a)]
    _, idx = np.unique(a, return_index=True)
    return a[np.sort(idx)]


def log_uniform(rng, lo, hi, n, dt):
    return (10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)).astype(dt)


def sincos_points(dt, rng):
    lim, kmax = (1e9, 29) if dt is F64 else (1e4, 12)
    half_pi = mp.pi / 2
    ks = list(range(40)) + [2 ** j for j in range(6, kmax + 1)] + [int(mp.floor(mp.mpf(lim) / half_pi))]
    pts = []
    for k in ks:                                            # k pi/2 rounded, +-1, 2, 3: the reduced argument is the rounding error
        pts += nbrs(rnd(k * half_pi, dt), 3, dt)
    for j in list(range(10)) + [100, 2 ** (kmax - 2)]:      # odd multiples of pi/4: the quadrant changes, |r| is at the kernels' edge
        pts += nbrs(rnd((2 * j + 1) * mp.pi / 4, dt), 2, dt)
    pts += nbrs(np.nextafter(dt(lim), dt(0)), 1, dt)
    tiny = np.finfo(dt).tiny
    pts += [dt(0), np.nextafter(dt(0), dt(1)), tiny, np.nextafter(tiny, dt(0)), tiny * dt(0.01), dt(1e-30), dt(1e-8), dt(1e5 - 1), dt(2e5),
            dt(3e7), dt(9.9e8)]
    pts += list(np.abs(np.concatenate([rng.uniform(-4, 4, 60), rng.uniform(-300, 300, 60), rng.normal(0, 1e-3, 20)])))
    pts += list(log_uniform(rng, 1e-12, lim * 0.999, 40, F64))
    x = uniq(pts, dt, lambda a: (a >= 0) & (a < dt(lim)))
    big = np.finfo(dt).max
    edge = np.array([lim, -lim, np.nextafter(dt(lim), dt(np.inf)), 4e12, -4e12, big, -big, np.inf, -np.inf, np.nan], dtype=dt)
    ref = [[mp.sin(mp.mpf(float(v))) for v in x], [mp.cos(mp.mpf(float(v))) for v in x]]
    return x, ref, edge


def rcp_points(dt, rng):
    fi = np.finfo(dt)
    emin, emax = fi.minexp, -fi.minexp                      # x = 2^emin .. 2^emax: normal x with a normal reciprocal
    pts = []
    for e in sorted(set(list(range(emin, emax + 1, 64 if dt is F64 else 9)) + [emin, emin + 1, -1, 0, 1, emax - 1, emax])):
        pts += nbrs(np.ldexp(dt(1), e), 2, dt)               # powers of two and their neighbours (beyond the ends: filtered below)
    eps = fi.eps
    for e in (-100, -1, 0, 100):
        pts += [np.ldexp(dt(2) - dt(j) * eps, e) for j in range(1, 5)]          # mantissas just below 2
    pts += nbrs(dt(1), 4, dt)
    pts += [dt(3), dt(1) / dt(3), dt(10), dt(0.1), dt(1.5), dt(1.4142135623730951), dt(1.9), dt(1.1)]
    pts += list(log_uniform(rng, 1e-12, 1e12, 200, dt))
    lo, hi = np.ldexp(dt(1), emin), np.ldexp(dt(1), emax)
    x = uniq(pts, dt, lambda a: (a >= lo) & (a <= hi))
    sub = fi.smallest_subnormal
    edge = [0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, np.nextafter(lo, dt(0)), lo / dt(4), np.nextafter(hi, dt(np.inf)), hi * dt(2),
            -hi * dt(2), fi.max, -fi.max]
    ref = [[1 / mp.mpf(float(v)) for v in x]]
    return x, ref, np.array(edge, dtype=dt)


def atan_points(dt, rng):
    fi = np.finfo(dt)
    pts = [dt(0)] + nbrs(dt(1), 4, dt)
    pts += [fi.smallest_subnormal, fi.tiny * dt(0.01), np.nextafter(fi.tiny, dt(0)), fi.tiny, dt(1e-30), dt(1e-17), dt(1e-9), dt(1e-8),
            dt(2.0 ** -27), dt(1e-5), dt(1e-3), dt(0.01), dt(0.1), dt(0.25), dt(0.5), dt(0.75), dt(0.999)]
    pts += [dt(2), dt(1e3), dt(1e5), dt(1e10), dt(1e16), dt(1e17), dt(2.0 ** 53), dt(1e30), np.ldexp(dt(1), -fi.minexp), fi.max / dt(4),
            fi.max / dt(2), np.nextafter(fi.max, dt(0)), fi.max]
    if dt is F64:
        pts += [dt(1e-310), dt(1e-300), dt(1e-200), dt(1e-100), dt(1e100), dt(1e300)]
    pts += list(np.abs(np.concatenate([rng.uniform(-60, 60, 100), rng.normal(0, 1, 60), rng.uniform(0.9, 1.1, 40), rng.uniform(-1, 1, 60)])))
    pts += list(log_uniform(rng, 1e-12, 1e12, 40, F64))
    x = uniq(pts, dt, lambda a: a >= 0)
    ref = [[mp.atan(mp.mpf(float(v))) for v in x]]
    return x, ref, np.array([np.inf, -np.inf, np.nan], dtype=dt)


def log_points(dt, rng):
    fi = np.finfo(dt)
    bits = fi.nmant
    pts = []
    for k in range(1, bits + 1):                            # 1 +- 2^-k: the compensated form near 1
        pts += [dt(1) + np.ldexp(dt(1), -k), dt(1) - np.ldexp(dt(1), -k)]
    pts += [dt(1), dt(1) - np.ldexp(dt(1), -bits - 1)]
    pts += nbrs(np.sqrt(dt(0.5)), 4, dt) + nbrs(np.sqrt(dt(2)), 4, dt)          # the frexp branch switches
    for e in (fi.minexp + 1, -64, -10, -1, 1, 2, 10, 64, fi.maxexp - 1):
        pts += nbrs(np.ldexp(dt(1), e), 1, dt)
    pts += [fi.tiny, np.nextafter(fi.tiny, dt(1)), fi.max, dt(np.e), dt(10), dt(0.1), dt(3)]
    edge = [0.0, -0.0, -1.0, -fi.tiny, -np.inf, np.inf, np.nan]
    sub = [fi.smallest_subnormal, fi.smallest_subnormal * dt(1000), fi.tiny * dt(0.01), np.nextafter(fi.tiny, dt(0))]
    if dt is F64:
        pts += sub                                          # fp64: frexp takes subnormals, the bound holds for them
        pts += list(log_uniform(rng, 1e-40, 1e4, 150, dt))
    else:
        edge += sub                                         # fp32: v_log_f32 is not specified for them
        pts += list(log_uniform(rng, 1e-30, 1e4, 150, dt))
    x = uniq(pts, dt, lambda a: a > 0)
    ref = [[mp.log(mp.mpf(float(v))) for v in x]]
    return x, ref, np.array(edge, dtype=dt)


def pow_points(dt, rng):
    p = [float(dt(S_THETA)), float(dt(S_PHI))]              # the exponent as the function is handed it
    f32 = np.finfo(F32)
    pts = [dt(1)] + nbrs(dt(1), 2, dt) + nbrs(dt(1e16), 2, dt) + [dt(2), dt(0.5), dt(10), dt(0.1), dt(1e-8), dt(1e8), dt(1e15), dt(9.9e15)]
    for q in p:                                             # the arguments at which x^q leaves the normal floats at the lower end
        for r in (0.25, 0.5, 0.9, 0.99, 0.999, 1.001, 1.01, 1.1, 2.0, 4.0):
            pts.append(rnd(mp.mpf(2) ** (mp.mpf(-126) / mp.mpf(q)) * r, dt))
    pts += [dt(f32.tiny), np.nextafter(F32(f32.tiny), F32(1)), dt(1e-37), dt(1e-35), dt(1e-30), dt(1e-20)]
    pts += list(log_uniform(rng, 1e-34, 1e16, 100, dt))
    pts += list(log_uniform(rng, 1e-8, 1e4, 60, F32).astype(dt))       # floats: the conversion of the fp64 overload is exact for them
    clamp = dt(1e16)
    x = uniq(pts, dt, lambda a: (a >= dt(f32.tiny)) & (a <= clamp))
    ref = []
    for q in p:
        row = [mp.mpf(float(v)) ** mp.mpf(q) for v in x]
        ref.append([r if mp.mpf(float(f32.tiny)) <= r <= mp.mpf(float(f32.max)) else None for r in row])
    big = np.finfo(dt).max
    edge = [0.0, -0.0, np.nextafter(clamp, dt(np.inf)), 1e17, 1e30, big, np.inf, -1.0, -np.inf, np.nan,
            f32.smallest_subnormal, 1e-40, np.nextafter(F32(f32.tiny), F32(0))]
    if dt is F64:
        edge += [1e-46, 1e-60, 1e-300, 5e-324, 1e100, 1e300]
    return x, ref, np.array(edge, dtype=dt)


def split(ref):
    """exact values -> (nearest double, (exact - hi) / ulp(hi) as float32)"""
    hi = np.full((len(ref), len(ref[0])), np.nan)
    lo = np.zeros(hi.shape, dtype=F32)
    for r, row in enumerate(ref):
        for i, v in enumerate(row):
            if v is None:
                continue
            h = float(v)
            hi[r, i] = h
            u = mp.mpf(float(np.spacing(abs(h))))
            lo[r, i] = F32(float((v - mp.mpf(h)) / u))
            assert abs(lo[r, i]) <= 0.5 + 1e-6, (r, i, h, lo[r, i])
    return hi, lo


def generate():
    makers = {"sincos": sincos_points, "frcp": rcp_points, "frcp1": rcp_points, "fatan": atan_points, "flog": log_points, "hpow": pow_points}
    arrays = {}
    for n, name in enumerate(FUNCS):
        dt = F64 if name.startswith("f64") else F32
        x, ref, edge = makers[name[4:]](dt, np.random.default_rng(20250611 + n))
        hi, lo = split(ref)
        arrays[name + ".x"] = x; arrays[name + ".hi"] = hi; arrays[name + ".lo"] = lo; arrays[name + ".edge"] = edge
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue(), compresslevel=9)
    return arrays, buf.getvalue()


def main():
    arrays, blob = generate()
    if "--check" in sys.argv[1:]:
        same = open(PATH, "rb").read() == blob
        print("math_edges.npz: %s" % ("reproduced byte for byte" if same else "DIFFERS from what the generator writes"))
        sys.exit(0 if same else 1)
    with open(PATH, "wb") as f:
        f.write(blob)
    print(", ".join("%s %d+%d" % (n, len(arrays[n + ".x"]), len(arrays[n + ".edge"])) for n in FUNCS))
    print("%d bytes" % len(blob))


if __name__ == "__main__":
    main()
