#!/usr/bin/env python3
"""Two checkouts' CPU builds of the solver core on the same inputs, compared word by word -- the check, without a GPU, that a change to
the sweeps of csrc/mpc_core.h leaves every bit where it was.

    python tools/twin_ab.py --old <checkout> --new <checkout> [--quick]

Each tree's tests/host_twin/*.cpp (with its csrc/mpc_params.cpp, which reads the configurations) is compiled into a temporary
directory with the flags of tests/certify_twin/Makefile -- hipcc's clang as a plain C++ compiler, -O2 -mfma -ffp-contract=on -- so
that the front end decides per expression which multiply-adds are fused, as it does for the device code.  (The suite's own
libhost_twin.so is a g++ build and stays what it is.)  Then every solve entry of both libraries runs on the same arrays:

    mpc_host_twin_solve, _solve_f32, _solve_mixed, _solve_mixed_f64, _solve_reparked (pass_cut 4), mpc_twin_solve cold, warm (from
    the cold call's buffer) and with a model column, mpc_horizon_twin_solve

on config-fast.json lake track B = 512 seed 21; config-stable.json N = 25 dt = 0.05 B = 64; N = 3; the weight sweep with velocity
weight 0; initial_state_rows = 1; max_soc = 4 on tests/golden/soc_instances.npz.  Prints words compared and words differing per
array; exit status 1 on any difference.  Nothing is loaded but the two pairs of twin libraries, and no environment is set.
--quick: a quarter of each lake-track batch."""
import argparse
import ctypes as C
import glob
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-x", "c++", "-O2", "-mfma", "-ffp-contract=on", "-std=c++17", "-fPIC", "-shared"]


def build(root, out_dir, tag):
    """-> (libhost_twin, libhorizon_twin) of the checkout `root`, both with that tree's parameter reader"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(root, "carnd-mpc-project_amd", "csrc")
    inc = ["-I", os.path.join(root, "include"), "-I", csrc]
    twin = os.path.join(root, "tests", "host_twin")
    horizon = os.path.join(twin, "horizon_twin.cpp")
    rest = sorted(p for p in glob.glob(os.path.join(twin, "*.cpp")) if p != horizon)
    libs = []
    for name, src in (("host", rest + [os.path.join(csrc, "mpc_params.cpp")]), ("horizon", [horizon])):
        out = os.path.join(out_dir, "lib%s_twin_%s.so" % (name, tag))
        subprocess.check_call([hipcc] + FLAGS + inc + ["-o", out] + src)
        libs.append(C.CDLL(out))
    return libs


def package(root):
    """the pure-Python part of the package of `root` (structures, scenarios); its native library is never loaded"""
    d = os.path.join(root, "carnd-mpc-project_amd")
    spec = importlib.util.spec_from_file_location("carnd_mpc_project_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["carnd_mpc_project_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None


class Runner:
    """the entries of one tree's pair of libraries, each returning {array name: array}"""

    def __init__(self, pkg, host, horizon):
        self.pkg, self.host, self.horizon = pkg, host, horizon

    def params(self, cfg, **over):
        p = self.pkg.MpcParams()
        rc = self.host.mpc_params_load_json(os.path.join(HERE, "tests", "golden", cfg).encode(), C.byref(p))
        assert rc == 0, (cfg, rc)
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def plain(self, entry, p, b, w, real=np.float64, extra=()):
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=real)
        st, cf, yl, yh, w = f(b["state"]), f(b["coeffs"]), f(b["yaw_lo"]), f(b["yaw_hi"]), f(w)
        B = st.shape[1]
        res = {"out": np.zeros((9, B), real), "traj": np.zeros((2 * p.N, B), real), "status": np.zeros(B, np.int32), "iters": np.zeros(B, np.int32)}
        more = {k: np.zeros(B, np.int32) for k in extra}
        rc = getattr(self.host, entry)(C.byref(p), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), vp(w), vp(res["out"]),
                                       vp(res["traj"]), vp(res["status"]), vp(res["iters"]), *[vp(a) for a in more.values()])
        assert rc == 0, (entry, rc)
        return dict(res, **more)

    def reparked(self, p, b, w, cut):
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        st, cf, yl, yh, w = f(b["state"]), f(b["coeffs"]), f(b["yaw_lo"]), f(b["yaw_hi"]), f(w)
        B = st.shape[1]
        res = {"out": np.zeros((9, B)), "status": np.zeros(B, np.int32), "iters": np.zeros(B, np.int32), "was_parked": np.zeros(B, np.int32)}
        rc = self.host.mpc_host_twin_solve_reparked(C.byref(p), C.c_int64(B), C.c_int64(B), C.c_int(cut), vp(st), vp(cf), vp(yl), vp(yh), vp(w),
                                                    vp(res["out"]), vp(res["status"]), vp(res["iters"]), vp(res["was_parked"]))
        assert rc == 0, rc
        return res

    def instance(self, p, b, w=None, model=None, warm=None, warm_status=None, opts=None, horizon=None):
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        st, cf, yl, yh, w, md, warm = f(b["state"]), f(b["coeffs"]), f(b["yaw_lo"]), f(b["yaw_hi"]), f(w), f(model), f(warm)
        B = st.shape[1]
        ws = None if warm_status is None else np.ascontiguousarray(warm_status, dtype=np.int32)
        res = {"out": np.zeros((9, B)), "traj": np.zeros((2 * p.N, B)), "status": np.zeros(B, np.int32), "iters": np.zeros(B, np.int32)}
        if opts is not None:                         # a warm call: the iterate comes back too
            res["warm"] = np.zeros(((p.N - 1) * self.pkg.WARM_REC, B))
        o = C.byref(opts) if opts is not None else None
        head = (C.byref(p), C.c_int64(B), C.c_int64(B), vp(st), vp(cf), vp(yl), vp(yh), vp(w), vp(md))
        tail = (vp(res["out"]), vp(res["traj"]), vp(res["status"]), vp(res["iters"]))
        if horizon is None:
            rc = self.host.mpc_twin_solve(*head, vp(warm), vp(ws), vp(res.get("warm")), C.c_int64(B), o, C.c_int(0), *tail)
        else:
            hz = np.ascontiguousarray(horizon, dtype=np.int32)
            rc = self.horizon.mpc_horizon_twin_solve(*head, vp(hz), vp(warm), vp(ws), vp(res.get("warm")), C.c_int64(B), o, *tail)
        assert rc == 0, rc
        return res

    def warm_opts(self):
        """mpc_warm_opts_default of the product library, which this tool does not load"""
        o = self.pkg.MpcWarmOpts()
        o.size, o.shift, o.mu_init, o.bound_push, o.duals = C.sizeof(self.pkg.MpcWarmOpts), 0, 1e-6, 1e-6, 0
        return o

    def everything(self, quick):
        """every (label, {array name: array}) of the stated entries and populations"""
        pkg = self.pkg
        gd = os.path.join(HERE, "tests", "golden")
        wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
        cut = 4 if quick else 1
        fast = self.params("config-fast.json")
        long_ = self.params("config-stable.json", N=25, dt=0.05)
        pops = [("config-fast B=%d" % (512 // cut), fast, 512 // cut, False), ("config-stable N=25 dt=0.05 B=%d" % (64 // cut), long_, 64 // cut, False),
                ("N=3", self.params("config-fast.json", N=3), 64 // cut, False), ("weight sweep, velocity weight 0", fast, 128 // cut, True),
                ("initial_state_rows=1", self.params("config-fast.json", initial_state_rows=1), 128 // cut, False)]
        for label, p, B, sweep in pops:
            b = pkg.scenarios.lake_track_batch(B, p, wp, seed=21)
            w = pkg.scenarios.weight_sweep(B, p, seed=22, velocity_weights=(0.0, 1.0, 100.0)) if sweep else None
            yield label + " solve", self.plain("mpc_host_twin_solve", p, b, w)
            yield label + " solve_f32", self.plain("mpc_host_twin_solve_f32", p, b, w, np.float32)
            yield label + " solve_mixed", self.plain("mpc_host_twin_solve_mixed", p, b, w, np.float32, extra=("iters_f32",))
            yield label + " solve_mixed_f64", self.plain("mpc_host_twin_solve_mixed_f64", p, b, w, extra=("iters_f32",))
            yield label + " solve_reparked pass_cut 4", self.reparked(p, b, w, 4)
            cold = self.instance(p, b, w, opts=self.warm_opts())
            yield label + " twin_solve cold", cold
            yield label + " twin_solve warm", self.instance(p, b, w, warm=cold["warm"], warm_status=cold["status"], opts=self.warm_opts())
            model = pkg.scenarios.model_rows(p, B)
            model[0] = np.random.default_rng(5).choice([0.05, 0.08, 0.1, 0.15], B)
            model[1] = np.random.default_rng(6).uniform(2.0, 3.5, B)
            yield label + " twin_solve model", self.instance(p, b, w, model=model)
            hz = np.random.default_rng(11).choice([n for n in (3, 4, 5, 7, 10, 13, 17, 25) if n <= p.N], B).astype(np.int32)
            yield label + " horizon_twin_solve", self.instance(p, b, w, model=model, horizon=hz)
        soc = np.load(os.path.join(gd, "soc_instances.npz"))
        for pop, cfg, over in (("n10", "config-fast.json", {}), ("n25", "config-stable.json", dict(N=25, dt=0.05))):     # tests/test_soc.py
            n = soc[pop + "_state"].shape[1] // cut
            b = {k: np.ascontiguousarray(soc["%s_%s" % (pop, k)][..., :n]) for k in ("state", "coeffs", "yaw_lo", "yaw_hi")}
            p = self.params(cfg, max_soc=4, initial_state_rows=1, max_iter=500, **over)
            yield "soc_instances %s max_soc=4 solve" % pop, self.plain("mpc_host_twin_solve", p, b, None)
            yield "soc_instances %s max_soc=4 twin_solve" % pop, self.instance(p, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True, help="checkout of the commit to compare with")
    ap.add_argument("--new", default=HERE, help="checkout under test (default: this one)")
    ap.add_argument("--quick", action="store_true", help="a quarter of each lake-track batch")
    a = ap.parse_args()
    pkg = package(HERE)
    with tempfile.TemporaryDirectory(prefix="twin_ab") as tmp:
        old = Runner(pkg, *build(os.path.abspath(a.old), tmp, "old"))
        new = Runner(pkg, *build(os.path.abspath(a.new), tmp, "new"))
        words = differ = 0
        for (label, ra), (_, rb) in zip(old.everything(a.quick), new.everything(a.quick)):
            for name in ra:
                x, y = ra[name], rb[name]
                bits = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
                bad = int((x.view(bits) != y.view(bits)).sum())
                words += x.size; differ += bad
                print("%-64s %-10s %8d words %6d differ   (status 0: %s)" % (label, name, x.size, bad, int((ra["status"] == 0).sum())))
    print("%d words compared, %d differ" % (words, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
