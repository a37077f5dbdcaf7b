#!/usr/bin/env python3
"""Registers / scratch / occupancy of every grouped forward kernel (cuembed_amd/csrc/c_api_grouped.hip) next to the
corresponding single-table instantiation (GatherReduceKernel with fp32 accumulation in c_api_forward.hip,
GatherReduceQuantizedKernel in c_api_quantized.hip), from hipcc's -Rpass-analysis=kernel-resource-usage remarks (as
tools/kernel_resources.py).  Instantiations are paired by their MANGLED template arguments and printed that way (the
demangler has no name for bf16).  No GPU needed; compiles the three units (a few minutes).

    python tools/grouped_forward_resources.py > profiles/grouped_forward_resources.txt
    python tools/grouped_forward_resources.py --tables     # the digit strings of grouped_gather_kernels.hpp

--tables prints the single-table kernels' occupancy in the order of kSingleTableWaves / kSingleTableWavesQuantized
(grouped_gather_kernels.hpp: the occupancy the grouped kernels are asked to hold).  A digit is lowered by hand where the
report shows that the grouped instantiation spills at it.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (r"\s(?:Total)?(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
          r"LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill): (\d+)")
GROUPED, GROUPED_Q = "25GatherReduceGroupedKernelI", "34GatherReduceQuantizedGroupedKernelI"
SINGLE, SINGLE_Q = "18GatherReduceKernelI", "27GatherReduceQuantizedKernelI"


def remarks(unit):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cuembed_amd", "csrc"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "cuembed_amd", "csrc", unit), "-o", "/dev/null"]
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
    """The mangled template arguments: between the kernel's name and the "EEv" that opens the parameter list."""
    i = name.index(kernel) + len(kernel)
    return name[i:name.index("EEv", i)]


def print_tables(single):
    """[element][IndexT 32/64][OffsetT 32/64][N: widest first][weighted][IndexSource], one digit each."""
    for kind, elems, widest in (("plain", (("f", 4), ("DF16_", 8), ("DF16b", 8)), None),
                                ("quantized", (("f", 16), ("DF16_", 16)), None)):
        digits = ""
        for elem, max_n in elems:
            for index in "il":
                for offset in "il":
                    for step in range(3):
                        for weighted in "01":
                            for source in "012":
                                acc = "f" if kind == "plain" else ""
                                prefix = "%s%s%s%sLi%dELb%sELNS0_11IndexSourceE%sE" % (elem, acc, index, offset,
                                                                                     max_n >> step, weighted, source)
                                match = [r for (k, a), r in single.items() if k == kind and a.startswith(prefix)]
                                assert len(match) == 1, prefix
                                digits += str(match[0]["Occupancy"])
        print(kind)
        for i in range(0, len(digits), 72):
            print('    "%s"' % digits[i:i + 72])
    return 0


def main():
    with ThreadPoolExecutor(max_workers=3) as ex:
        grouped, forward, quantized = ex.map(remarks, ["c_api_grouped.hip", "c_api_forward.hip", "c_api_quantized.hip"])
    single = {}
    for name, r in forward.items():
        if SINGLE in name:
            single[("plain", template_args(name, SINGLE))] = r
    for name, r in quantized.items():
        if SINGLE_Q in name:
            single[("quantized", template_args(name, SINGLE_Q))] = r
    if "--tables" in sys.argv:
        return print_tables(single)
    lines, below_by, spills = [], {}, 0
    for name, r in grouped.items():
        if GROUPED in name:
            args = template_args(name, GROUPED)
            elem = re.match(r"(f|DF16_|DF16b)(.*)", args)      # the single-table kernel has AccT = float behind ElemT
            key, kernel = ("plain", elem.group(1) + "f" + elem.group(2)), "GatherReduceGroupedKernel"
        elif GROUPED_Q in name:
            args = template_args(name, GROUPED_Q)
            key, kernel = ("quantized", args), "GatherReduceQuantizedGroupedKernel"
        else:
            continue
        s = single[key]
        spills += bool(r["ScratchSize"] or r["VGPRs Spill"] or r["SGPRs Spill"])
        step = s["Occupancy"] - r["Occupancy"]
        if step > 0:
            below_by[step] = below_by.get(step, 0) + 1
        lines.append("%-4d %-4d %-7d %-6d %-6d %-3d | %-4d %-4d %-3d %s %s<%s>" % (
            r["VGPRs"], r["SGPRs"], r["ScratchSize"], r["VGPRs Spill"], r["SGPRs Spill"], r["Occupancy"], s["VGPRs"],
            s["SGPRs"], s["Occupancy"], "BELOW" if step > 0 else "     ", kernel, args))
    below = sum(below_by.values())
    print(__doc__.split("\n\n")[0])
    print("Template arguments as mangled: f / DF16_ / DF16b = fp32 / fp16 / bf16, i / l = int32 / int64 (IndexT, OffsetT), LiN =")
    print("elements per lane, Lb0 / Lb1 = unweighted / weighted, IndexSourceE0 / 1 / 2 = LDS-staged / cross-lane / global.")
    print()
    print("%d instantiations; scratch or spills: %d; occupancy equal to or above the single-table instantiation: %d; below it: "
          "%d, marked BELOW (by 1 / 2 / 3 waves per SIMD: %d / %d / %d)" % (
              len(lines), spills, len(lines) - below, below, below_by.get(1, 0), below_by.get(2, 0), below_by.get(3, 0)))
    print()
    print("grouped                                | single-table")
    print("VGPR SGPR scratch Vspill Sspill occ | VGPR SGPR occ       kernel")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
