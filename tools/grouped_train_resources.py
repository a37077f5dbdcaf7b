#!/usr/bin/env python3
"""Registers / scratch / occupancy of the kernels that train a group beyond sum pooling (grouped_train_kernels.hpp:
WeightGradGroupedKernel, GroupedMeanScaleKernel, compiled in cuembed_amd/csrc/c_api_grouped_backward.hip) and of the
single-table WeightGradKernel (c_api_forward.hip), whose body the grouped kernel shares (WeightGradBag) -- from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (as tools/kernel_resources.py).  With --parent DIR, a checkout of the
parent commit, WeightGradKernel's instantiations are listed for both trees side by side: sharing the body must not
change them.  Instantiations are printed by their MANGLED template arguments (the demangler has no name for bf16).
No GPU needed; compiles two units per tree (a few minutes).

    git worktree add /tmp/parent HEAD~1
    python tools/grouped_train_resources.py --parent /tmp/parent > profiles/grouped_train_kernel_resources.txt
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (r"\s(?:Total)?(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
          r"LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill): (\d+)")
NEW = (("WeightGradGroupedKernel", "23WeightGradGroupedKernelI"), ("GroupedMeanScaleKernel", "22GroupedMeanScaleKernelI"))
SINGLE = "16WeightGradKernelI"
COLUMNS = ("VGPRs", "SGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "Occupancy")


def remarks(root, unit):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "cuembed_amd", "csrc"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(root, "cuembed_amd", "csrc", unit), "-o", "/dev/null"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(FIELDS, line)
        if m and cur:
            rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


def template_args(name, kernel):
    i = name.index(kernel) + len(kernel)
    return name[i:name.index("EEv", i)]


def pick(rows, kernel):
    return {template_args(n, kernel): r for n, r in rows.items() if kernel in n}


def cells(r):
    return " ".join("%-7d" % r[c] for c in COLUMNS)


def main():
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    jobs = [(ROOT, "c_api_grouped_backward.hip"), (ROOT, "c_api_forward.hip")]
    if parent:
        jobs.append((parent, "c_api_forward.hip"))
    with ThreadPoolExecutor(max_workers=3) as ex:
        results = list(ex.map(lambda j: remarks(*j), jobs))
    print(__doc__.split("\n\n")[0])
    print("Template arguments as mangled: f / DF16_ / DF16b = fp32 / fp16 / bf16, i / l = int32 / int64 (IndexT, OffsetT),")
    print("LiN = elements per lane, Lb0 / Lb1 = unweighted / weighted.  Columns: VGPRs, SGPRs, scratch bytes per lane,")
    print("VGPR spills, SGPR spills, waves per SIMD.")
    bad = 0
    for label, kernel in NEW:
        found = pick(results[0], kernel)
        assert found, kernel
        scratch = sum(1 for r in found.values() if r["ScratchSize"] or r["VGPRs Spill"] or r["SGPRs Spill"])
        bad += scratch
        print("\n%s: %d instantiations; scratch or spills: %d" % (label, len(found), scratch))
        print("VGPR    SGPR    scratch Vspill  Sspill  occ      kernel")
        for args, r in found.items():
            print("%s  %s<%s>" % (cells(r), label, args))
    here = pick(results[1], SINGLE)
    assert here, SINGLE
    print("\nWeightGradKernel (single table): %d instantiations on this tree" % len(here))
    if parent:
        before = pick(results[2], SINGLE)
        differ = sorted(a for a in set(here) | set(before) if here.get(a) != before.get(a))
        bad += len(differ)
        print("on the parent commit: %d; instantiations whose figures differ: %d%s"
              % (len(before), len(differ), "" if not differ else "  " + " ".join(differ)))
        print("this tree                                        | parent commit")
        print("VGPR    SGPR    scratch Vspill  Sspill  occ      | VGPR    SGPR    scratch Vspill  Sspill  occ      kernel")
        for args, r in here.items():
            print("%s | %s  WeightGradKernel<%s>" % (cells(r), cells(before[args]) if args in before else "-", args))
    else:
        print("VGPR    SGPR    scratch Vspill  Sspill  occ      kernel")
        for args, r in here.items():
            print("%s  WeightGradKernel<%s>" % (cells(r), args))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
