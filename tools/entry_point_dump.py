#!/usr/bin/env python3
"""Every batch entry point in every form on one build, written to one .npz -- and two such files compared word by word.

  python tools/entry_point_dump.py --root <a checkout, built> --out a.npz      # needs an MI355X
  python tools/entry_point_dump.py --compare a.npz b.npz

What runs is what tests/test_entry_points_gpu.py runs (tests/entry_point_forms.py of THIS checkout, on the package and library of
--root): every form at B = 5 on a default config-fast.json handle and at B = 70 with wave_max_batch = -1 (host forms and the wire
form: B = 3), at ld = B and at ld = B + 3 / ld_warm = B + 2, the rollouts with and without hist; every row of the refusal table
with its code and text; and one solve_torch and one solve_numpy at B = 8192, where the take order and lane compaction are in play,
with take_order_info()["launches_in_key_order"] after the two.  --compare prints the arrays and words compared and how many
differ, and whether the refusal tables are the same; exit status 1 if anything differs."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(root, out):
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
    np.savez_compressed(out, __refusals__=np.array(json.dumps(refusals)), **arrays)
    words = sum(a.size for a in arrays.values())
    print("%s: %d arrays, %d words, %d refusal rows, launches_in_key_order %d" %
          (out, len(arrays), words, len(refusals), int(arrays["launches_in_key_order B=8192"][0])))


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
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.root, a.out))


if __name__ == "__main__":
    main()
