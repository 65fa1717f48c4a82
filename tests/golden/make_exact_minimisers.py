#!/usr/bin/env python3
"""Generate tests/golden/exact_minimisers.npz: EXACT minimisers of the reference NLP, for every form of the solve.

What the SLSQP cross-solves (make_golden.py) are to the plain solve at 1e-6, this file is to every entry point at the accuracy
of the oracle itself: the minimiser of the NLP to 30 digits, rounded to double, found without one derivative formula.

Method (all arithmetic in mpmath at 70 digits):
  * The NLP is restated from MPC.cpp (objective :68-114 with every `if` decided at the start point, model rows :116-153, bounds
    :222-257) -- the branch outcomes and the bounds through make_golden.Problem, the rest below -- and from the words of
    include/mpc_amd.h for the per-instance forms: a model column replaces dt, Lf and the four limits, the speed target is
    computeSpeedTarget on the HANDLE's tables capped by the COLUMN's max_speed; a horizon n is the reference with Config::N = n.
  * Single shooting: the model rows are explicit recurrences, so only the 2 (N-1) controls are unknowns; the state follows by
    rollout.  Controls on a bound are fixed at the CALLER's bound (not the relaxed one); psi / v bounds that are active enter as
    equalities with multipliers.  The Lagrangian's gradient is a central difference (h = 1e-25), its Hessian a second difference
    (h = 1e-17); Newton with that matrix runs until the step is below 1e-30.
  * The multipliers of the model rows come from one linear solve with the differenced Jacobian of the full-space rows, and the
    stationarity of the controls in the full space is then asserted (1e-25): two routes to the same bound multipliers.
  * The oracle's solution serves as the starting guess and names the active set, nothing else: whatever the guess, a point is
    admitted only if, in this arithmetic, Newton converged, every active bound has a multiplier >= 1e-3 of the right sign, every
    inactive bound is >= 1e-5 away, the reduced Hessian on the free controls is positive definite, and the oracle ends the
    instance with SUCCESS.  Candidates that fail are replaced by the next draw and counted.
  * For 24 cases the primal-dual point is stored as a record in MPC_WARM_REC layout (duals times df), with a perturbed copy, and
    for both the rows of the certificate as include/mpc_amd_certify.h words them, computed at the ROUNDED doubles by differences.

Per class the yardstick of a quantity is 8 x the oracle's largest distance to the exact value, at least 4 ulp of max(1, |exact|)
(the rule of make_fit_edges.py); the script asserts that none exceeds TOL_STEER / TOL_ACCEL / TOL_TRAJ of tests/helpers.py.

Run:  python tests/golden/make_exact_minimisers.py [-j PROCESSES]     (needs mpmath, scipy through make_golden.py, the oracle and the built package; about a minute on 8 cores)
"""
import io
import json
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_golden as MG  # noqa: E402

mp.mp.dps = 70
H1 = mp.mpf(10) ** -25          # gradient step: truncation ~1e-50, rounding ~1e-45
H2 = mp.mpf(10) ** -17          # second differences: truncation ~1e-34, rounding ~1e-36
STEP_TOL = mp.mpf(10) ** -30
MIN_MULT, MIN_DIST = 1e-3, 1e-5
MODEL_FIELDS = ("dt", "Lf", "max_steering", "max_acceleration", "max_deceleration", "max_speed")
MODEL_KEYS = ("dt", "Lf", "max_steering", "max_acc", "max_dec", "max_speed")      # the same six in make_golden's config dict
CLASSES = ("plain", "a_free", "v_bound", "horizons", "weights", "model", "mixed_horizon")
QUANT = ("steer", "accel", "state", "traj", "cost")
WARM_REC = 22
NMAX = 25
RELAX = 1e-8                    # MpcParams.bound_relax_factor's default
TOLS = dict(tol=1e-8, dual_inf_tol=1.0, constr_viol_tol=1e-4, compl_inf_tol=1e-4, acceptable_tol=1e-6,
            acceptable_dual_inf_tol=1e10, acceptable_constr_viol_tol=1e-2, acceptable_compl_inf_tol=1e-2)   # MpcParams' defaults
CONVERGED, ACCEPTABLE, NOT_CONVERGED, NOT_A_POINT = 0, 1, 2, 3
COST_GROUPS = ((0, 11), (1, 10), (2, 9), (3,), (4,))


def M(x):
    return mp.mpf(float(x))


def case_config(cs):
    """make_golden's config dict for a case: the handle's file, N / dt of the handle, then the case's weights, model column, horizon."""
    c = MG.load_config(cs["config"])
    c["N"], c["dt"] = int(cs["N"]), float(cs["dt"])
    if cs.get("max_speed") is not None:                   # a handle whose max_speed was overridden after Config::load: the tables stay as loaded
        c["max_speed"] = float(cs["max_speed"])
    if cs.get("weights") is not None:
        c["w"] = [float(v) for v in cs["weights"]]
    if cs.get("model") is not None:                       # mpc_amd.h: the six values of the column; the speed tables stay the handle's
        for k, v in zip(MODEL_KEYS, cs["model"]):
            c[k] = float(v)
    if cs.get("horizon") is not None:                     # mpc_amd_horizon.h: the reference with Config::N = horizon
        c["N"] = int(cs["horizon"])
    return c


class ExactNLP:
    """The NLP of one instance in mpmath.  Full-space vectors are lists in the reference's quantity-major layout (MPC.cpp:56-63)."""

    def __init__(self, c, state, coef, yaw_lo, yaw_hi):
        P = self.P = MG.Problem(c, state, coef, yaw_lo, yaw_hi)        # branch outcomes at the start point, bounds, layout
        self.N, self.n, self.ix = P.N, P.n, P.ix
        self.dt, self.Lf = M(c["dt"]), M(c["Lf"])
        self.w = [M(v) for v in c["w"]]
        self.state = [M(v) for v in state]
        self.coef = [M(v) for v in coef]
        self.lo, self.hi = [float(v) for v in P.lo], [float(v) for v in P.hi]

    # -- the two functions of MPC.cpp -----------------------------------------------------------------------------------------
    def f(self, z, keep=None):
        """MPC.cpp:68-114 on the frozen tape; keep: the weights that count (a cost group), None = all"""
        P, N, I = self.P, self.N, self.ix
        w = self.w if keep is None else [v if q in keep else mp.mpf(0) for q, v in enumerate(self.w)]
        s = mp.mpf(0)
        for i in range(N):
            cte, epsi, v = z[I["cte"] + i], z[I["epsi"] + i], z[I["v"] + i]
            s += (w[0] if abs(P.xi[I["cte"] + i]) < P.c["cte_panic"] else w[11]) * cte * cte
            s += (w[10] if abs(P.xi[I["epsi"] + i]) > P.c["epsi_panic"] else w[1]) * epsi * epsi
            d = v - M(P.vref[i])
            s += w[2] * d * d
            if P.negv[i]:
                s += w[9] * v * v
        for i in range(N - 1):
            dl, a = z[I["delta"] + i], z[I["a"] + i]
            s += w[3] * dl * dl
            if P.apos[i]:
                s += w[6] * a * a
            if P.declow[i]:
                d = z[I["v"] + i] - a
                s += w[8] * d * d
        for i in range(N - 2):
            d = z[I["delta"] + i + 1] - z[I["delta"] + i]
            s += w[4] * d * d
            if P.dapos[i]:
                d = z[I["a"] + i + 1] - z[I["a"] + i]
                s += w[7] * d * d
        return s

    def step(self, x0, y0, psi0, v0, cte0, epsi0, d0, a0):
        """the right-hand sides of MPC.cpp:141-152"""
        co = self.coef
        vdt = v0 * self.dt
        psi = psi0 + d0 * vdt / self.Lf
        fx = mp.mpf(0)
        fpx = mp.mpf(0)
        for k in range(len(co) - 1, -1, -1):
            fx = fx * x0 + co[k]
        for k in range(len(co) - 1, 0, -1):
            fpx = fpx * x0 + k * co[k]
        return (x0 + mp.cos(psi0) * vdt, y0 + mp.sin(psi0) * vdt, psi, v0 + a0 * self.dt, (fx - y0) + mp.sin(epsi0) * vdt,
                psi - mp.atan(fpx))

    def g(self, z):
        """the model rows of index 1 .. N-1 (MPC.cpp:122-153), row (q, i) at q (N-1) + i-1"""
        N, I = self.N, self.ix
        names = ("x", "y", "psi", "v", "cte", "epsi")
        r = [None] * (6 * (N - 1))
        for i in range(1, N):
            rhs = self.step(*[z[I[q] + i - 1] for q in names], z[I["delta"] + i - 1], z[I["a"] + i - 1])
            for q, nm in enumerate(names):
                r[q * (N - 1) + i - 1] = z[I[nm] + i] - rhs[q]
        return r

    def rollout(self, u):
        """controls u = delta_0.., a_0.. -> the full vector whose model rows are zero"""
        N, I = self.N, self.ix
        names = ("x", "y", "psi", "v", "cte", "epsi")
        z = [mp.mpf(0)] * self.n
        for q, nm in enumerate(names):
            z[I[nm]] = self.state[q]
        for i in range(N - 1):
            z[I["delta"] + i], z[I["a"] + i] = u[i], u[N - 1 + i]
        for i in range(1, N):
            rhs = self.step(*[z[I[q] + i - 1] for q in names], u[i - 1], u[N - 1 + i - 1])
            for q, nm in enumerate(names):
                z[I[nm] + i] = rhs[q]
        return z

    # -- the active-set Newton iteration ----------------------------------------------------------------------------------------
    def solve(self, sol, act_tol=1e-6):
        """sol: a double-precision solution (the oracle's): starting guess and active set.  -> dict, or a string saying why not."""
        N, I = self.N, self.ix
        nu = 2 * (N - 1)
        uvar = [I["delta"] + i for i in range(N - 1)] + [I["a"] + i for i in range(N - 1)]
        fixed, sact = {}, []                                # control j -> (bound, +1 upper / -1 lower); (var index, bound, sign)
        for j, vi in enumerate(uvar):
            if sol[vi] >= self.hi[vi] - act_tol:
                fixed[j] = (M(self.hi[vi]), 1)
            elif sol[vi] <= self.lo[vi] + act_tol:
                fixed[j] = (M(self.lo[vi]), -1)
        for nm in ("psi", "v"):
            for i in range(1, N):
                vi = I[nm] + i
                if sol[vi] >= self.hi[vi] - act_tol:
                    sact.append((vi, M(self.hi[vi]), 1))
                elif sol[vi] <= self.lo[vi] + act_tol:
                    sact.append((vi, M(self.lo[vi]), -1))
        free = [j for j in range(nu) if j not in fixed]
        u0 = [fixed[j][0] if j in fixed else M(sol[uvar[j]]) for j in range(nu)]
        nf, m = len(free), len(sact)

        def lagr(u, mu):
            z = self.rollout(u)
            s = self.f(z)
            for (vi, b, sg), t in zip(sact, mu):
                s += t * sg * (z[vi] - b)
            return s

        def lagr_w(wv):
            u = list(u0)
            for t, j in enumerate(free):
                u[j] = wv[t]
            return lagr(u, wv[nf:])

        def grad(fun, x, idx, h=H1):
            out = []
            for i in idx:
                xp, xm = list(x), list(x)
                xp[i] += h; xm[i] -= h
                out.append((fun(xp) - fun(xm)) / (2 * h))
            return out

        wv = [u0[j] for j in free] + [mp.mpf(0)] * m
        nw = nf + m

        def hessian(wv):
            """second differences of the Lagrangian; the block of the multipliers is zero (it is linear in them)"""
            K = mp.zeros(nw, nw)
            L0 = lagr_w(wv)
            for i in range(nf):
                for j in range(i, nw):
                    if i == j:
                        xp, xm = list(wv), list(wv)
                        xp[i] += H2; xm[i] -= H2
                        K[i, i] = (lagr_w(xp) - 2 * L0 + lagr_w(xm)) / (H2 * H2)
                    else:
                        v4 = []
                        for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                            x = list(wv)
                            x[i] += si * H2; x[j] += sj * H2
                            v4.append(lagr_w(x))
                        K[i, j] = K[j, i] = (v4[0] - v4[1] - v4[2] + v4[3]) / (4 * H2 * H2)
            return K
        # Newton with the matrix of the guess (a chord iteration: the guess is 1e-8 away, so every step gains ~8 digits); with active
        # state bounds the matrix is taken once more after the first step, when their multipliers are known
        K = hessian(wv)
        steps = []
        try:
            for it in range(30):
                gr = grad(lagr_w, wv, range(nw))
                dw = mp.lu_solve(K, mp.matrix([-t for t in gr]))
                wv = [a + dw[t] for t, a in enumerate(wv)]
                steps.append(max([abs(dw[t]) for t in range(nw)] + [mp.mpf(0)]))
                if steps[-1] < STEP_TOL:
                    break
                if it == 0 and m:
                    K = hessian(wv)
        except ZeroDivisionError:
            return "singular KKT matrix"
        if steps[-1] >= STEP_TOL:
            return "Newton did not converge (last step %s)" % mp.nstr(steps[-1], 3)
        u = list(u0)
        for t, j in enumerate(free):
            u[j] = wv[t]
        mu = wv[nf:]
        z = self.rollout(u)
        # bound multipliers of the fixed controls: the Lagrangian's slope against the bound
        gfix = grad(lambda x: lagr(x, mu), u, sorted(fixed))
        zc = {j: -fixed[j][1] * gfix[t] for t, j in enumerate(sorted(fixed))}       # upper: -dL/du, lower: +dL/du
        mults = [float(v) for v in zc.values()] + [float(t) for t in mu]
        min_mult = min(mults) if mults else float("inf")
        if min_mult < MIN_MULT:
            return "an active bound's multiplier is %.3g" % min_mult
        dist = float("inf")
        held = set(vi for vi, _, _ in sact) | set(uvar[j] for j in fixed)
        for vi in uvar + [I[nm] + i for nm in ("psi", "v") for i in range(1, N)]:
            if vi not in held:
                dist = min(dist, float(z[vi]) - self.lo[vi], self.hi[vi] - float(z[vi]))
        if dist < MIN_DIST:
            return "an inactive bound is %.3g away" % dist
        # the reduced Hessian on the free controls (null space of the active rows), from the converged K
        Kf = np.array([[float(K[i, j]) for j in range(nw)] for i in range(nw)])
        Hf, A = Kf[:nf, :nf], Kf[nf:, :nf]
        if m:
            _, sv, vt = np.linalg.svd(A)
            if sv.min() < 1e-9 * sv.max():
                return "active rows are dependent"
            Z = vt[m:].T
            Hr = Z.T @ Hf @ Z
        else:
            Hr = Hf
        eig = float(np.linalg.eigvalsh(Hr).min()) if Hr.size else float("inf")
        if eig <= 1e-9 * max(1.0, float(np.abs(Hf).max())):
            return "reduced Hessian not positive definite (min eigenvalue %.3g)" % eig
        # model-row multipliers in the full space: J_s^T lam = -(grad_s f - zL_s + zU_s)
        svar = [I[nm] + i for nm in ("x", "y", "psi", "v", "cte", "epsi") for i in range(1, N)]
        gf = grad(self.f, z, svar + uvar)
        cols = []
        for vi in svar + uvar:
            zp, zm = list(z), list(z)
            zp[vi] += H1; zm[vi] -= H1
            gp, gm = self.g(zp), self.g(zm)
            cols.append([(a - b) / (2 * H1) for a, b in zip(gp, gm)])
        ns = len(svar)
        zL, zU = [mp.mpf(0)] * self.n, [mp.mpf(0)] * self.n
        for (vi, b, sg), t in zip(sact, mu):
            (zU if sg > 0 else zL)[vi] = t
        for j, t in zc.items():
            (zU if fixed[j][1] > 0 else zL)[uvar[j]] = t
        JsT = mp.matrix(ns, ns)
        for c_, col in enumerate(cols[:ns]):
            for r_ in range(ns):
                JsT[c_, r_] = col[r_]
        rhs = mp.matrix([-(gf[t] - zL[vi] + zU[vi]) for t, vi in enumerate(svar)])
        lam = mp.lu_solve(JsT, rhs)
        worst = mp.mpf(0)
        for t, vi in enumerate(uvar):                       # the controls' stationarity in the full space: the second route to zc
            r = gf[ns + t] + sum(cols[ns + t][r_] * lam[r_] for r_ in range(ns)) - zL[vi] + zU[vi]
            worst = max(worst, abs(r))
        assert worst < mp.mpf(10) ** -25, ("full-space stationarity of the controls", mp.nstr(worst, 5))
        assert max(abs(t) for t in self.g(z)) < mp.mpf(10) ** -60
        return {"z": z, "lam": [lam[t] for t in range(ns)], "zL": zL, "zU": zU, "J": self.f(z), "min_mult": min_mult, "min_dist": dist,
                "red_eig": eig, "newton_steps": len(steps), "last_step": float(steps[-1]),
                "fixed": {uvar[j]: fixed[j][1] for j in fixed}, "sact": {vi: sg for vi, _, sg in sact}}

    # -- the record and the certificate ---------------------------------------------------------------------------------------
    def objective_scaling(self):
        """IPOPT's gradient-based scaling at the start point: 100 / max |grad f(xi)| where that is below 1 (at least 1e-8)"""
        xi = [M(v) for v in self.P.xi]
        gmax = mp.mpf(0)
        for i in range(self.n):
            xp, xm = list(xi), list(xi)
            xp[i] += H1; xm[i] -= H1
            gmax = max(gmax, abs((self.f(xp) - self.f(xm)) / (2 * H1)))
        return mp.mpf(1) if gmax <= 100 else max(100 / gmax, mp.mpf(10) ** -8)

    def record(self, s, df):
        """the primal-dual point in MPC_WARM_REC layout, duals times df, rounded to double: [(N-1) * 22]"""
        N, I = self.N, self.ix
        rec = np.zeros((N - 1, WARM_REC))
        for k in range(N - 1):
            for q, nm in enumerate(("x", "y", "psi", "v", "cte", "epsi")):
                rec[k, q] = float(s["z"][I[nm] + k + 1])
                rec[k, 8 + q] = float(df * s["lam"][q * (N - 1) + k])
            rec[k, 6], rec[k, 7] = float(s["z"][I["delta"] + k]), float(s["z"][I["a"] + k])
            for b, vi in enumerate((I["psi"] + k + 1, I["v"] + k + 1, I["delta"] + k, I["a"] + k)):
                rec[k, 14 + b], rec[k, 18 + b] = float(df * s["zL"][vi]), float(df * s["zU"][vi])
        return rec.reshape(-1)

    def certificate(self, rec):
        """The rows of include/mpc_amd_certify.h at a record of doubles, in this arithmetic and by differences -> (rows [12], sizes, verdict)."""
        N, I = self.N, self.ix
        rec = np.asarray(rec, dtype=np.float64).reshape(N - 1, WARM_REC)
        z = [mp.mpf(0)] * self.n
        names = ("x", "y", "psi", "v", "cte", "epsi")
        for q, nm in enumerate(names):
            z[I[nm]] = self.state[q]
        lam = [mp.mpf(0)] * (6 * (N - 1))
        zL, zU = [mp.mpf(0)] * self.n, [mp.mpf(0)] * self.n
        bounded = []
        for k in range(N - 1):
            for q, nm in enumerate(names):
                z[I[nm] + k + 1] = M(rec[k, q])
                lam[q * (N - 1) + k] = M(rec[k, 8 + q])
            z[I["delta"] + k], z[I["a"] + k] = M(rec[k, 6]), M(rec[k, 7])
            for b, vi in enumerate((I["psi"] + k + 1, I["v"] + k + 1, I["delta"] + k, I["a"] + k)):
                zL[vi], zU[vi] = M(rec[k, 14 + b]), M(rec[k, 18 + b])
                bounded.append(vi)
        df = self.objective_scaling()
        rows = [mp.mpf(0)] * 12
        rows[0] = self.f(z)
        for t, keep in enumerate(COST_GROUPS):
            rows[7 + t] = self.f(z, keep)
        rows[6] = df
        lo = {vi: M(self.lo[vi]) for vi in bounded}
        hi = {vi: M(self.hi[vi]) for vi in bounded}
        rows[5] = max([mp.mpf(0)] + [max(lo[vi] - z[vi], z[vi] - hi[vi]) for vi in bounded])
        rl = {vi: lo[vi] - M(RELAX) * max(1, abs(lo[vi])) for vi in bounded}
        rh = {vi: hi[vi] + M(RELAX) * max(1, abs(hi[vi])) for vi in bounded}
        inside = all(rl[vi] <= z[vi] <= rh[vi] for vi in bounded)
        X = max(1.0, max(abs(float(t)) for t in z))
        Lam = max(1.0, max(abs(float(t)) for t in lam), max(float(t) for t in zL), max(float(t) for t in zU))
        sizes = {"X": X, "Lam": Lam, "df": float(df), "inside": inside}
        if not inside:
            out = np.full(12, np.nan); out[5] = float(rows[5])
            sizes.update(sd=1.0, sc=1.0)
            return out, sizes, NOT_A_POINT
        g = self.g(z)
        cinf = max(abs(t) for t in g)

        def phi(zz):
            gg = self.g(zz)
            return df * self.f(zz) + sum(a * b for a, b in zip(lam, gg))
        held = [I[nm] + i for nm in names for i in range(1, N)] + [I["delta"] + i for i in range(N - 1)] + [I["a"] + i for i in range(N - 1)]
        dinf = mp.mpf(0)
        for vi in held:
            zp, zm = list(z), list(z)
            zp[vi] += H1; zm[vi] -= H1
            dinf = max(dinf, abs((phi(zp) - phi(zm)) / (2 * H1) - zL[vi] + zU[vi]))
        prods = [(z[vi] - rl[vi]) * zL[vi] for vi in bounded] + [(rh[vi] - z[vi]) * zU[vi] for vi in bounded]
        cmax, cmin = max(prods), min(prods)
        lsum, zsum = sum(abs(t) for t in lam), sum(zL[vi] + zU[vi] for vi in bounded)
        mrows, nb, smax = 6 * (N - 1), 8 * (N - 1), 100
        sd = max(smax, (lsum + zsum) / (mrows + nb)) / smax
        sc = max(smax, zsum / nb) / smax
        E0 = max(dinf / sd, cinf, max(abs(cmax), abs(cmin)) / sc)
        rows[1], rows[2], rows[3], rows[4] = cinf, dinf / df, cmax / df, E0
        sizes.update(sd=float(sd), sc=float(sc))
        T = TOLS
        if E0 <= T["tol"] and rows[2] <= T["dual_inf_tol"] and cinf <= T["constr_viol_tol"] and rows[3] <= T["compl_inf_tol"]:
            verdict = CONVERGED
        elif (E0 <= T["acceptable_tol"] and rows[2] <= T["acceptable_dual_inf_tol"] and cinf <= T["acceptable_constr_viol_tol"]
              and rows[3] <= T["acceptable_compl_inf_tol"]):
            verdict = ACCEPTABLE
        else:
            verdict = NOT_CONVERGED
        return np.array([float(t) for t in rows]), sizes, verdict

    def perturbed(self, rec):
        """the fixed perturbation: delta_0 + 1e-3 where that stays inside the relaxed box, x_2 + 1e-4, every lam of stage 1 + 1e-2"""
        r = np.array(rec, dtype=np.float64, copy=True).reshape(self.N - 1, WARM_REC)
        hi = self.hi[self.ix["delta"]]
        if r[0, 6] + 1e-3 <= hi + RELAX * max(1.0, abs(hi)):
            r[0, 6] += 1e-3
        r[1, 0] += 1e-4
        r[1, 8:14] += 1e-2
        return r.reshape(-1)


# ---- one candidate ------------------------------------------------------------------------------------------------------------------
def oracle_solve(cs):
    import oracle_lib as O
    over = {"N": int(cs["horizon"] if cs.get("horizon") is not None else cs["N"]), "dt": float(cs["dt"])}
    if cs.get("max_speed") is not None:
        over["max_speed"] = float(cs["max_speed"])
    if cs.get("model") is not None:
        over.update({k: float(v) for k, v in zip(MODEL_FIELDS, cs["model"])})
    cfg = O.load_config(cs["config"], **over)
    cfg.yaw_low, cfg.yaw_high = float(cs["yaw_lo"]), float(cs["yaw_hi"])
    if cs.get("weights") is not None:
        for q in range(12):
            cfg.weights[q] = float(cs["weights"][q])
    st, o9, tx, ty, info, sol = O.mpc_solve(cfg, cs["state"], cs["coef"], want_sol=True)
    return st, o9, np.concatenate([tx, ty]), sol


def work(cs):
    """-> (case, result dict) or (case, reason string)"""
    mp.mp.dps = 70
    st, o9, otraj, sol = oracle_solve(cs)
    if st != 0:
        return cs, "the oracle ends with status %d" % st
    nlp = ExactNLP(case_config(cs), cs["state"], cs["coef"], cs["yaw_lo"], cs["yaw_hi"])
    s = nlp.solve(sol)
    if isinstance(s, str):
        return cs, s
    N, I = nlp.N, nlp.ix
    if cs["cls"] == "a_free" and any(vi >= I["a"] for vi in s["fixed"]):
        return cs, "an acceleration sits on its bound"
    if cs["cls"] == "v_bound" and not any(I["v"] <= vi < I["v"] + N for vi in s["sact"]):
        return cs, "no speed bound is active"
    need = cs.get("need")
    if need == "a_max" and s["fixed"].get(I["a"]) != 1:
        return cs, "a_0 is not on max_acceleration"
    if need == "a_min" and s["fixed"].get(I["a"]) != -1:
        return cs, "a_0 is not on max_deceleration"
    if need == "steer" and I["delta"] not in s["fixed"]:
        return cs, "delta_0 is not on max_steering"
    z = s["z"]
    out9 = np.array([float(z[I[q] + 1]) for q in ("x", "y", "psi", "v", "cte", "epsi")] + [float(z[I["delta"]]), float(z[I["a"]]), float(s["J"])])
    traj = np.array([float(z[I["x"] + i]) for i in range(N)] + [float(z[I["y"] + i]) for i in range(N)])
    act = np.zeros((4, NMAX - 1), dtype=np.int8)
    for k in range(N - 1):
        for b, vi in enumerate((I["psi"] + k + 1, I["v"] + k + 1, I["delta"] + k, I["a"] + k)):
            act[b, k] = s["sact"].get(vi, 0) or s["fixed"].get(vi, 0)
    res = {"out": out9, "traj": traj, "act": act, "margins": np.array([s["min_mult"], s["min_dist"], s["red_eig"]]),
           "ref_err": np.concatenate([np.abs(o9 - out9), [np.abs(otraj - traj).max()]]), "n": N, "newton_steps": s["newton_steps"]}
    # the cap: 8 x the oracle's distance is the class yardstick, and no yardstick may exceed today's tolerances (tests/helpers.py:
    # TOL_STEER, TOL_ACCEL 1e-6; TOL_TRAJ 1e-5 for the step-1 state and the trajectory).  Long arcs on a psi bound do: the oracle holds
    # psi 1e-8 outside the caller's bound (bound_relax_factor) and the far end of the trajectory drifts by that angle times the distance.
    e = res["ref_err"]
    if 8 * max(e[6], e[7]) > 1e-6 or 8 * max(e[:6].max(), e[9]) > 1e-5:
        return cs, "8 x the oracle's distance exceeds today's tolerance (steer %.2e accel %.2e state %.2e traj %.2e)" % (e[6], e[7], e[:6].max(), e[9])
    if cs.get("want_record"):
        df = nlp.objective_scaling()
        rec = nlp.record(s, df)
        rows0, sz0, v0 = nlp.certificate(rec)
        pert = nlp.perturbed(rec)
        rows1, sz1, v1 = nlp.certificate(pert)
        res["record"] = {"rec": rec, "pert": pert, "rows": np.stack([rows0, rows1]), "verdict": [v0, v1],
                         "sizes": np.array([[sz[k] for k in ("X", "Lam", "df", "sd", "sc")] for sz in (sz0, sz1)])}
    return cs, res


# ---- the candidates -----------------------------------------------------------------------------------------------------------------
def candidates(pkg):
    """[(class, wanted, [candidate cases in the order they are tried])]"""
    G = lambda name: os.path.join(HERE, name)
    wp = pkg.scenarios.load_waypoints(G("lake_track_waypoints.csv"))
    fast = pkg.params_from_json(G("config-fast.json"))
    base = lambda cls, name, config, N, dt, state, coef, ylo, yhi, **kw: dict(
        cls=cls, name=name, config=config, N=int(N), dt=float(dt), state=[float(v) for v in state], coef=[float(v) for v in coef],
        yaw_lo=float(ylo), yaw_hi=float(yhi), **kw)

    def lake(cls, tag, params, n, seed, **kw):
        b = pkg.scenarios.lake_track_batch(n, params, wp, seed=seed)
        return [base(cls, "%s-%d" % (tag, i), "config-fast.json", params.N, params.dt, b["state"][:, i], b["coeffs"][:, i], b["yaw_lo"][i], b["yaw_hi"][i], **kw)
                for i in range(n)]

    def straight(cls, tag, config, v0, c0, theta=0.0, c2=0.0, **kw):
        c = MG.load_config(config)
        c1 = float(np.tan(theta))
        return base(cls, tag, config, c["N"], c["dt"], [0.0, 0.0, 0.0, v0, c0, -float(np.arctan(c1))], [c0, c1, c2, 0.0, 0.0], -0.1, 0.1, **kw)
    groups = []
    gold = json.load(open(G("scipy_cross_solve.json")))["cases"]
    plain = []
    for t, c in enumerate(gold):
        cfg = MG.load_config(c["config"])
        plain.append(base("plain", c["name"], c["config"], cfg["N"], cfg["dt"], c["state"], c["coef"], c["yaw_lo"], c["yaw_hi"],
                          want_record=t in (0, 1, 5, 9, 13, 25, 29, 33)))
    groups.append(("plain", 37, plain))
    # a_free and v_bound.  On the configs as they are the speed target of every stage from 1 on IS max_speed (steer_speeds[0], capped by
    # Config::load), and v_{N-1} enters the objective through (v - target)^2 alone: wherever a_{N-2} is free, v_{N-1} sits on its bound
    # with a multiplier of exactly zero.  No such instance can pass the admission test (strict complementarity), whatever the road; the
    # v_bound candidates below show it and are all rejected.  a_free therefore runs on handles whose max_speed is raised to 1.25 x the
    # file's AFTER the load (the override params_from_json and mpc_main.cpp's command line apply): the table keeps the file's cap, the
    # target lies inside the speed box and all nine accelerations are free with every bound far away.
    offs = [(0.3, 0.0), (-0.5, 0.01), (0.8, -0.02), (-1.1, 0.0), (0.15, -0.01), (-0.25, 0.02)]
    af, vb = [], []
    for config in ("config-stable.json", "config-fast.json"):
        c = MG.load_config(config)
        vref = MG.speed_target(c, 0.0, c["max_speed"])
        for t, (c0, th) in enumerate(offs):
            af.append(straight("a_free", "afree-%s-%d" % (config[7:-5], t), config, vref - 0.05, c0, th, want_record=t < 2, max_speed=1.25 * c["max_speed"]))
            if t < 4:
                vb.append(straight("v_bound", "vbound-%s-%d" % (config[7:-5], t), config, c["max_speed"] - 0.004 * (t + 1), c0, th))
    groups.append(("a_free", 10, af))
    groups.append(("v_bound", 8, vb))
    hz = []
    for n, cnt, seed in ((3, 6, 84), (4, 5, 85), (17, 5, 86)):
        hz += lake("horizons", "lake-N%d" % n, pkg.params_from_json(G("config-fast.json"), N=n), cnt, seed)
    for cs in hz[:4]:
        cs["want_record"] = True
    ext = json.load(open(G("scipy_cross_solve_ext.json")))["cases"]
    for t, c in enumerate(c for c in ext if c["N"] == 25):
        hz.append(base("horizons", c["name"], c["config"], 25, 0.05, c["state"], c["coef"], c["yaw_lo"], c["yaw_hi"], want_record=t < 2))
    groups.append(("horizons", len(hz), hz))                 # every one wanted; a reject shrinks the class (at least 6 asserted)
    ws = [base("weights", c["name"], c["config"], 10, 0.1, c["state"], c["coef"], c["yaw_lo"], c["yaw_hi"], weights=c["weights"])
          for c in ext if c["weights"] is not None]
    more = pkg.scenarios.weight_sweep(8, fast, seed=81, velocity_weights=(1.0, 100.0))
    for t, cs in enumerate(lake("weights", "lake-weights-b", fast, 8, 81)):
        cs["weights"] = more[:, t].tolist()
        ws.append(cs)
    groups.append(("weights", len(ws), ws))
    own = np.array([getattr(fast, k) for k in MODEL_FIELDS])
    md = []
    for t, (cs, fa) in enumerate(zip(lake("model", "model-amax", fast, 8, 87), (0.6, 1.3, 0.8, 1.7, 0.5, 1.5, 0.7, 1.2))):
        col = own * np.array([(0.8, 1.0, 1.2, 0.5)[t % 4], (1.1, 0.9)[t % 2], 1.0, fa, (0.7, 1.4)[t % 2], 1.0])
        cs.update(model=col.tolist(), need="a_max", want_record=t < 3)
        md.append(cs)
    for t, (c0, v0) in enumerate(((2.0, 5.0), (-2.5, 6.0), (3.0, 4.0), (-1.8, 7.0), (2.6, 8.0), (-3.0, 5.5), (1.6, 4.5), (-2.2, 6.5))):
        col = own * np.array([1.0, (1.0, 1.15)[t % 2], 1.0, 1.0, 1.0, 1.0]); col[2] = 0.002
        md.append(straight("model", "model-steer-%d" % t, "config-fast.json", v0, c0, model=col.tolist(), need="steer", want_record=t < 2))
    for t, cs in enumerate(lake("model", "model-vmax", fast, 12, 88)):
        col = own * np.array([1.0, 1.0, (0.8, 1.2)[t % 2], 1.0, 1.0, 0.7])
        if abs(cs["state"][3]) < col[5] - 0.5:
            cs.update(model=col.tolist(), need="vmax", want_record=len([c for c in md if c.get("need") == "vmax"]) < 1)
            md.append(cs)
    # a_0 on the column's max_deceleration, on both sides of the handle's: a curve met at 1 m/s below the speed target brakes at the limit
    # (the column's max_speed is 1.25 x the handle's, so that the target lies inside the speed box: see a_free above)
    for t, (c0, th, c2, fd) in enumerate(((0.3, 0.0, 0.012, 0.7), (0.3, 0.0, 0.012, 1.4), (0.3, 0.03, 0.008, 1.4), (1.0, 0.03, 0.012, 0.7), (1.0, 0.0, 0.012, 1.4),
                                          (0.3, 0.0, -0.008, 0.7))):
        col = own * np.array([1.0, 1.0, 1.0, 1.0, fd, 1.25])
        md.append(straight("model", "model-amin-%d" % t, "config-fast.json", own[5] - 1.0, c0, th, c2=c2, model=col.tolist(), need="a_min"))
    groups.append(("model", {"a_max": 5, "steer": 5, "vmax": 3, "a_min": 3}, md))
    mh = lake("mixed_horizon", "mixed", fast, 24, 89)
    for t, cs in enumerate(mh):
        cs["horizon"] = 3 + t % 8
        col = own * (np.array([0.8, 1.1, 0.9, 0.8, 1.2, 1.0]) if t % 2 else 1.0)
        cs["model"] = col.tolist()
    groups.append(("mixed_horizon", 16, mh))
    return groups


def main():
    import __graft_entry__ as Gm
    import helpers as Hh
    pkg = Gm.load_package()          # scenario generators (pure numpy) and the JSON loader only
    jobs = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else min(8, os.cpu_count() or 1)
    groups = candidates(pkg)
    allc = [cs for _, _, lst in groups for cs in lst]
    with multiprocessing.Pool(jobs) as pool:
        done = []
        for cs, res in pool.imap(work, allc, chunksize=1):
            done.append((cs, res))
            print("%-14s %-22s %s" % (cs["cls"], cs["name"], res if isinstance(res, str) else
                                       "admitted: Newton %d steps, multiplier >= %.3g, inactive >= %.3g, oracle d_steer %.2e d_state %.2e d_traj %.2e" %
                                       (res["newton_steps"], res["margins"][0], res["margins"][1], res["ref_err"][6], res["ref_err"][:6].max(), res["ref_err"][9])), flush=True)
    admitted, rejected = [], 0
    for cls, want, lst in groups:
        left = dict(want) if isinstance(want, dict) else {None: want}
        for cs in lst:
            cs2, res = done[allc.index(cs)]
            if isinstance(res, str):
                rejected += 1
                continue
            key = cs.get("need") if isinstance(want, dict) else None
            if left.get(key, 0) > 0:
                left[key] -= 1
                admitted.append((cs, res))
        if cls in ("plain",):
            assert left[None] == 0, "every input of scipy_cross_solve.json must be admitted"
    print("rejected candidates: %d of %d; admitted %d" % (rejected, len(allc), len(admitted)))
    n = len(admitted)
    assert n <= 160
    per = {c: [t for t, (cs, _) in enumerate(admitted) if cs["cls"] == c] for c in CLASSES}
    classes = [c for c in CLASSES if per[c] or c != "v_bound"]
    if not per["v_bound"]:
        print("v_bound: none of the %d candidates admitted -- the class is left out (see candidates())" % len(dict((g[0], g[2]) for g in groups)["v_bound"]))
    for c in classes:
        assert len(per[c]) >= 6, (c, len(per[c]))
    mdl = [admitted[t][0] for t in per["model"]]
    assert sum(c["need"] == "a_max" for c in mdl) >= 4 and sum(c["need"] == "steer" for c in mdl) >= 4 and sum(c["need"] == "vmax" for c in mdl) >= 2 and sum(c["need"] == "a_min" for c in mdl) >= 2
    # the yardsticks
    eps = np.finfo(float).eps
    yard = {}
    for c in classes:
        e = np.array([admitted[t][1]["ref_err"] for t in per[c]])
        o = np.array([admitted[t][1]["out"] for t in per[c]])
        tr = max(np.abs(admitted[t][1]["traj"]).max() for t in per[c])
        yard[c] = {"steer": max(8 * e[:, 6].max(), 4 * eps * max(1.0, np.abs(o[:, 6]).max())),
                   "accel": max(8 * e[:, 7].max(), 4 * eps * max(1.0, np.abs(o[:, 7]).max())),
                   "state": max(8 * e[:, :6].max(), 4 * eps * max(1.0, np.abs(o[:, :6]).max())),
                   "traj": max(8 * e[:, 9].max(), 4 * eps * max(1.0, tr)),
                   "cost": max(8 * (e[:, 8] / np.maximum(1.0, np.abs(o[:, 8]))).max(), 4 * eps)}
        print("yardsticks %-14s %s   (%d cases)" % (c, "  ".join("%s %.3g" % (q, yard[c][q]) for q in QUANT), len(per[c])))
        assert yard[c]["steer"] <= Hh.TOL_STEER and yard[c]["accel"] <= Hh.TOL_ACCEL and yard[c]["state"] <= Hh.TOL_TRAJ and yard[c]["traj"] <= Hh.TOL_TRAJ, c
    # arrays
    A = {"state": np.zeros((6, n)), "coef": np.zeros((5, n)), "yaw": np.zeros((2, n)), "weights": np.full((12, n), np.nan),
         "model": np.full((6, n), np.nan), "horizon": np.zeros(n, dtype=np.int32), "N": np.zeros(n, dtype=np.int32), "dt": np.zeros(n), "max_speed": np.full(n, np.nan),
         "cls": np.zeros(n, dtype=np.int8), "config": np.zeros(n, dtype=np.int8), "out": np.zeros((9, n)), "traj": np.full((2 * NMAX, n), np.nan),
         "act": np.zeros((4, NMAX - 1, n), dtype=np.int8), "margins": np.zeros((3, n)), "ref_err": np.zeros((10, n))}
    configs = ("config-stable.json", "config-fast.json")
    recs = []
    for t, (cs, r) in enumerate(admitted):
        A["state"][:, t], A["coef"][:, t], A["yaw"][:, t] = cs["state"], cs["coef"], (cs["yaw_lo"], cs["yaw_hi"])
        if cs.get("weights") is not None:
            A["weights"][:, t] = cs["weights"]
        if cs.get("model") is not None:
            A["model"][:, t] = cs["model"]
        A["horizon"][t] = cs.get("horizon") or 0
        A["max_speed"][t] = cs.get("max_speed") or np.nan
        A["N"][t], A["dt"][t], A["cls"][t], A["config"][t] = cs["N"], cs["dt"], classes.index(cs["cls"]), configs.index(cs["config"])
        k = r["n"]
        A["out"][:, t] = r["out"]; A["traj"][:k, t] = r["traj"][:k]; A["traj"][NMAX:NMAX + k, t] = r["traj"][k:]
        A["act"][:, :, t], A["margins"][:, t], A["ref_err"][:, t] = r["act"], r["margins"], r["ref_err"]
        if "record" in r:
            recs.append((t, r["record"]))
    # part 3: 24 records.  The verdict at the exact point is the one the header's rule gives on the exact rows: where a quantity sits
    # on the CALLER's bound its slack against the RELAXED bound is bound_relax_factor max(1, |b|), and slack x dual puts E_0 between
    # 1e-8 and 2e-6 (ACCEPTABLE or NOT_CONVERGED); CONVERGED only where no bound is active (a_free).  A record is kept if E_0 is not
    # within 1 % of a threshold (so that no rounding decides the verdict) and its perturbed copy is NOT_CONVERGED or NOT_A_POINT.
    clear = lambda e: all(abs(e / t - 1.0) > 0.01 for t in (TOLS["tol"], TOLS["acceptable_tol"]))
    good = [(t, rc) for t, rc in recs if clear(rc["rows"][0][4]) and rc["verdict"][1] in (NOT_CONVERGED, NOT_A_POINT)
            and (rc["verdict"][1] == NOT_A_POINT or clear(rc["rows"][1][4]))]
    print("records: %d computed, %d kept; verdicts at the exact points: %s" % (len(recs), len(good), np.bincount([rc["verdict"][0] for _, rc in good], minlength=3).tolist()))
    for t, rc in good:
        print("   %-18s exact: verdict %d E_0 %.3g   perturbed: verdict %d E_0 %.3g" % (admitted[t][0]["name"], rc["verdict"][0], rc["rows"][0][4], rc["verdict"][1], rc["rows"][1][4]))
    for cs, r in admitted:
        if cs["cls"] == "a_free" and "record" in r:
            assert r["record"]["verdict"][0] == CONVERGED, cs["name"]
    good = good[:24]
    assert len(good) == 24, len(good)
    A["rec_case"] = np.array([t for t, _ in good], dtype=np.int32)
    A["rec"] = np.full((2, (NMAX - 1) * WARM_REC, 24), np.nan)
    A["rec_rows"] = np.zeros((2, 12, 24)); A["rec_sizes"] = np.zeros((2, 5, 24)); A["rec_verdict"] = np.zeros((2, 24), dtype=np.int8)
    for j, (t, rc) in enumerate(good):
        for v, key in enumerate(("rec", "pert")):
            A["rec"][v, :len(rc[key]), j] = rc[key]
        A["rec_rows"][:, :, j], A["rec_sizes"][:, :, j], A["rec_verdict"][:, j] = rc["rows"], rc["sizes"], rc["verdict"]
    meta = {"generator": "tests/golden/make_exact_minimisers.py", "digits": mp.mp.dps, "classes": list(classes), "configs": list(configs),
            "quantities": list(QUANT), "names": [cs["name"] for cs, _ in admitted], "yardsticks": yard, "rejected": rejected,
            "margins": ["smallest multiplier of an active bound", "smallest distance of an inactive bound", "smallest eigenvalue of the reduced Hessian"],
            "ref_err": "rows 0-8: |oracle - exact| of out, row 9: of the trajectory", "rec_sizes": ["X", "Lam", "df", "sd", "sc"]}
    A["meta"] = np.array(json.dumps(meta))
    buf = io.BytesIO()
    np.savez_compressed(buf, **A)
    path = os.path.join(HERE, "exact_minimisers.npz")
    open(path, "wb").write(buf.getvalue())
    print("wrote %s: %d cases, %d bytes" % (path, n, len(buf.getvalue())))
    assert len(buf.getvalue()) < 200 * 1024
    worst = A["ref_err"]
    print("oracle vs exact, all classes: d_steer %.3g  d_accel %.3g  d_state %.3g  d_traj %.3g  d_cost(rel) %.3g" %
          (worst[6].max(), worst[7].max(), worst[:6].max(), worst[9].max(), (worst[8] / np.maximum(1.0, np.abs(A["out"][8]))).max()))


if __name__ == "__main__":
    main()
