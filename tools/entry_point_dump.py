#!/usr/bin/env python3
"""Every batch entry point in every form on one build, written to one .npz -- and two such files compared word by word.

  python tools/entry_point_dump.py --root <a checkout, built> --out a.npz [--lanes]     # needs an MI355X
  python tools/entry_point_dump.py --compare a.npz b.npz

What runs is what tests/test_entry_points_gpu.py runs (tests/entry_point_forms.py of THIS checkout, on the package and library of
--root): every form at B = 5 on a default config-fast.json handle and at B = 70 with wave_max_batch = -1 (host forms and the wire
form: B = 3), at ld = B and at ld = B + 3 / ld_warm = B + 2, the rollouts with and without hist; every row of the refusal table
with its code and text; and one solve_torch and one solve_numpy at B = 8192, where the take order and lane compaction are in play,
with take_order_info()["launches_in_key_order"] after the two.  --lanes adds the phases of the lane kernel at B = 8192 + 11 (see
lanes()).  --compare prints the arrays and words compared and how many differ, and whether the refusal tables are the same; exit
status 1 if anything differs."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(root, out, with_lanes=False):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import entry_point_forms as E
    import __graft_entry__ as G
    import torch
    assert torch.cuda.is_available(), "the dump needs a GPU"
    pkg = G.load_package()
    dev = torch.device("cuda:0")
    gd = os.path.join(HERE, "tests", "golden")
    fast = pkg.params_from_json(os.path.join(gd, "config-fast.json"))
    wp = pkg.scenarios.load_waypoints(os.path.join(gd, "lake_track_waypoints.csv"))
    arrays, refusals = {}, []

    def keep(label, results):
        for k, r in enumerate(results):
            assert r["rc"] == 0 and r["pad"], (label, k, r["rc"], r["msg"], r["pad"])
            for name, a in r.items():
                if name not in ("rc", "msg", "pad"):
                    arrays["%s #%d %s" % (label, k, name)] = a
    for family in E.FAMILIES:
        shapes = [(5, fast), (70, E.with_params(fast, wave_max_batch=-1))] if family in E.DEVICE else [(3, fast)]
        for B, params in shapes:
            d = E.cars(pkg, fast, wp, B)
            with pkg.BatchedMPC(params, B, device=0) as mpc:
                for form in E.forms_of(family):
                    for hist in ((True, False) if family in E.ROLLOUT else (True,)):
                        for ld, ldw in ((B, B), (B + 3, B + 2)):
                            keep("%s%s B=%d ld=%d hist=%d" % (family, form, B, ld, hist),
                                 E.sequence(pkg, mpc, dev, family, form, d, hist=hist, ld=ld, ld_warm=ldw))
    d16 = E.cars(pkg, fast, wp, E.B16)
    for handle, how in E.HANDLES.items():
        with pkg.BatchedMPC(E.with_params(fast, **how), E.B16, device=0) as mpc:
            refusals += [[label, rc, text] for label, rc, text, _, _ in E.refusal_calls(pkg, mpc, dev, d16, handle)]
    B = 8192
    b = pkg.scenarios.lake_track_batch(B, fast, wp)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        res = mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), want_traj=True)
        mpc.tail_wait()
        torch.cuda.synchronize()
        host = mpc.solve_numpy(b["state"], b["coeffs"], b["yaw_lo"], b["yaw_hi"], want_traj=True)
        for k in ("out", "traj", "status", "iters"):
            arrays["solve_torch B=8192 " + k] = res[k].cpu().numpy()
            arrays["solve_numpy B=8192 " + k] = host[k]
        arrays["launches_in_key_order B=8192"] = np.array([mpc.take_order_info()["launches_in_key_order"]], dtype=np.int32)
    if with_lanes:
        lanes(pkg, torch, dev, fast, wp, arrays)
    np.savez_compressed(out, __refusals__=np.array(json.dumps(refusals)), **arrays)
    words = sum(a.size for a in arrays.values())
    print("%s: %d arrays, %d words, %d refusal rows, launches_in_key_order %d" %
          (out, len(arrays), words, len(refusals), int(arrays["launches_in_key_order B=8192"][0])))


def lanes(pkg, torch, dev, fast, wp, arrays):
    """The phases of the lane kernel, which the forms above do not reach, at the smallest batches the host lets them run (multi-phase
    solve and lane compaction from 8192, deferred tails from 4096): cut schedule, deferred tails, both mixed-precision modes with the
    promoted iterates in their columns and in their buffer, SOC, the automatic fp32 start of a long horizon.  Each case is recorded
    only after its path is seen to have run: iterations beyond the cut, a deferred batch, tail slices."""
    def solve(label, q, B, seed, sweep=False, staging=None, ran=None):
        b = pkg.scenarios.lake_track_batch(B, q, wp, seed=seed)
        w = pkg.scenarios.weight_sweep(B, q, seed=seed + 1, velocity_weights=(0.0, 1.0, 100.0)) if sweep else None
        dt_ = torch.float32 if q.precision == pkg.PRECISION_F32 else torch.float64
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt_)
        old = os.environ.get("MPC_STAGING")
        if staging is not None:
            os.environ["MPC_STAGING"] = staging
        try:
            with pkg.BatchedMPC(q, B, device=0) as mpc:
                r = mpc.solve_torch(t(b["state"]), t(b["coeffs"]), t(b["yaw_lo"]), t(b["yaw_hi"]), weights=None if w is None else t(w), want_traj=True)
                mpc.tail_wait()
                torch.cuda.synchronize()
                info = mpc.tail_info()
        finally:
            if staging is not None:
                os.environ.pop("MPC_STAGING", None)
                if old is not None:
                    os.environ["MPC_STAGING"] = old
        res = {k: v.cpu().numpy() for k, v in r.items()}
        it_max = int(res["iters"].max())
        print("lanes %-44s B %5d  iters.max %3d  success %.4f  batches_deferred %d  slices %d" %
              (label, B, it_max, float((res["status"] == 0).mean()), info["batches_deferred"], info["tail_launches"]), flush=True)
        assert ran is None or ran(it_max, info), (label, it_max, info)
        for k in ("out", "traj", "status", "iters"):
            arrays["lanes %s %s" % (label, k)] = res[k]

    B = 8192 + 11
    base = fast.copy(); base.N = 10; base.dt = 0.1

    def cuts(q):
        q.f64_f32_start = 0; q.pass_cut = 4
        for k in range(3):
            q.pass_cut_next[k] = 4
        return q
    beyond = lambda cut: (lambda it_max, info: it_max > cut)
    solve("pass_cut 4,4,4,4", cuts(base.copy()), B, 201, ran=beyond(16))
    solve("pass_cut 4,4,4,4 MPC_STAGING=0", cuts(base.copy()), B, 201, staging="0", ran=beyond(16))
    q = base.copy(); q.f64_f32_start = 0; q.tail_cut = 14
    solve("tail_cut 14, weights", q, B, 203, sweep=True, ran=lambda it_max, info: it_max > 14 and info["batches_deferred"] > 0 and info["tail_launches"] > 0)
    for refill in (0, 1):
        q = base.copy(); q.f64_f32_start = 1; q.f32_phase_refill = refill
        solve("f64_f32_start 1, f32_phase_refill %d" % refill, q, B, 205, ran=beyond(0))
    for finish in (1, 0):
        q = base.copy(); q.precision = pkg.PRECISION_F32; q.f32_finish = finish
        solve("PRECISION_F32, weights, f32_finish %d" % finish, q, B, 207, sweep=True, ran=beyond(0))
    q = cuts(base.copy()); q.max_soc = 4
    solve("pass_cut 4,4,4,4 max_soc 4", q, B, 201, ran=beyond(16))
    q = fast.copy(); q.N = 25; q.dt = 0.05
    assert q.f64_f32_start == 2                    # MPC_F32_START_AUTO: in effect from N = 15
    solve("N=25 dt=0.05 automatic fp32 start", q, 4096 + 11, 209, ran=beyond(0))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    ra, rb = json.loads(str(a["__refusals__"])), json.loads(str(b["__refusals__"]))
    names = sorted((set(a.files) | set(b.files)) - {"__refusals__"})
    words = differ = missing = 0
    for name in names:
        if name not in a.files or name not in b.files or a[name].shape != b[name].shape or a[name].dtype != b[name].dtype:
            missing += 1
            print("only in one file, or another shape:", name)
            continue
        x, y = a[name], b[name]
        bits = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
        bad = int((np.ascontiguousarray(x).view(bits) != np.ascontiguousarray(y).view(bits)).sum())
        words += x.size; differ += bad
        if bad:
            print("%d of %d words differ: %s" % (bad, x.size, name))
    rows_differ = sum(1 for x, y in zip(ra, rb) if x != y) + abs(len(ra) - len(rb))
    for x, y in zip(ra, rb):
        if x != y:
            print("refusal differs:", x, "|", y)
    print("%d arrays, %d words compared, %d differ; %d arrays without a partner; %d refusal rows, %d differ" %
          (len(names), words, differ, missing, len(ra), rows_differ))
    return 0 if differ == 0 and missing == 0 and rows_differ == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library run")
    ap.add_argument("--out", default="entry_points.npz")
    ap.add_argument("--lanes", action="store_true", help="also the phases of the lane kernel: cuts, deferred tails, mixed precision (see lanes())")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.root, a.out, a.lanes))


if __name__ == "__main__":
    main()
