#!/usr/bin/env python3
"""Compare the device code of two builds of csrc/mpc_solver.hip kernel by kernel, after normalising what a new template argument
changes without changing an instruction: the mangled names and the numbering of local labels.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=on -std=c++17 -Iinclude -Icarnd-mpc-project_amd/csrc --cuda-device-only -S \\
          -o new.s carnd-mpc-project_amd/csrc/mpc_solver.hip            (and the same on the other commit -> old.s)
    tools/isa_compare.py old.s new.s [--json out.json]

Prints, per kernel of old.s, "same" or the first differing line, then the register / scratch / LDS table of every kernel of new.s
(from the .amdhsa_ directives).  Exit status 1 if a kernel of old.s is missing from new.s or differs."""
import json
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (body lines, {directive: value})}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.section", text, re.S | re.M):
        out[m.group(1)] = [m.group(2), {}]
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        if m.group(1) in out:
            out[m.group(1)][1] = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, res))


def key(name):
    """the demangled name without what only the newer build has: mpc_solve_kernel is known by its first eight template arguments
    (further ones that are `false` -- HORIZON, DRIVE -- are a newer build's; its last parameter's type spells the same arguments out
    again)"""
    m = re.search(r"mpc_solve_kernel<([^()]*?)>\(", name)
    if not m:
        return name
    args = m.group(1).split(", ")
    while len(args) > 8 and args[-1] == "false":
        args.pop()
    return "mpc_solve_kernel<%s>" % ", ".join(args)


def normalise(body, own):
    lines = []
    labels = {}
    for ln in body.split("\n"):
        ln = ln.split(";")[0].rstrip()
        if not ln.strip() or ln.strip().startswith((".p2align", ".loc", ".file", ".cfi")):
            continue
        ln = ln.replace(own, "@self")
        ln = re.sub(r"\.LBB\d+_(\d+)", lambda m: ".L%d" % labels.setdefault(m.group(0), len(labels)), ln)
        ln = re.sub(r"_Z\w+", "@sym", ln)
        lines.append(ln)
    return lines


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    old, new = kernels(args[0]), kernels(args[1])
    dn_old, dn_new = demangle(list(old)), demangle(list(new))
    by_key = {key(dn_new[n]): n for n in new}
    bad = 0
    report = {"same": [], "differs": [], "missing": [], "resources": {}}
    for n, (body, _) in sorted(old.items(), key=lambda kv: dn_old[kv[0]]):
        k = key(dn_old[n])
        if k not in by_key:
            print("MISSING  %s" % dn_old[n]); bad += 1; report["missing"].append(dn_old[n]); continue
        a, b = normalise(body, n), normalise(new[by_key[k]][0], by_key[k])
        if a == b:
            print("same     %6d lines  %s" % (len(a), dn_old[n][:150])); report["same"].append(dn_old[n])
        else:
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("DIFFERS  at line %d of %d / %d  %s\n   old: %s\n   new: %s" % (at, len(a), len(b), dn_old[n][:150], a[at:at + 1], b[at:at + 1]))
            bad += 1; report["differs"].append(dn_old[n])
    print()
    print("%-9s %-9s %-8s %-8s  kernel" % ("vgpr", "sgpr", "scratch", "LDS"))
    for n, (_, d) in sorted(new.items(), key=lambda kv: dn_new[kv[0]]):
        row = {"next_free_vgpr": d.get("next_free_vgpr"), "accum_offset": d.get("accum_offset"), "next_free_sgpr": d.get("next_free_sgpr"),
               "scratch_bytes": d.get("private_segment_fixed_size"), "static_lds_bytes": d.get("group_segment_fixed_size")}
        report["resources"][dn_new[n]] = row
        print("%-9s %-9s %-8s %-8s  %s" % (row["next_free_vgpr"], row["next_free_sgpr"], row["scratch_bytes"], row["static_lds_bytes"], dn_new[n][:170]))
    for a in sys.argv[1:]:
        if a.startswith("--json="):
            json.dump(report, open(a[7:], "w"), indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
