#!/usr/bin/env python3
"""Registers / scratch / occupancy of every 4-bit mixed-width forward kernel (GatherReduceQuantized4BitMixedGroupKernel,
cuembed_amd/csrc/c_api_quantized_mixed_group_fourbit.hip) next to the single-table 4-bit instantiations of the same
output, index and offset types, codes per lane and weighting (GatherReduceQuantized4BitKernel in
c_api_quantized_fourbit.hip), from hipcc's -Rpass-analysis=kernel-resource-usage remarks (as
tools/quantized_mixed_group_forward_resources.py).  A staged instantiation has one counterpart (indices staged in LDS);
an unstaged one holds BOTH CSR walks -- the choice is made per workgroup at run time -- so it is listed next to the
cross-lane and the global-load instantiation.  No GPU needed; compiles two units.

    python tools/quantized_4bit_mixed_group_forward_resources.py > profiles/quantized_4bit_mixed_group_forward_resources.txt
"""
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grouped_forward_resources import remarks, template_args  # noqa: E402

KERNEL, SINGLE_KERNEL = "GatherReduceQuantized4BitMixedGroupKernel", "GatherReduceQuantized4BitKernel"
MIXED, SINGLE = ("%d%sI" % (len(k), k) for k in (KERNEL, SINGLE_KERNEL))


def main():
    with ThreadPoolExecutor(max_workers=2) as ex:
        mixed, fourbit = ex.map(remarks, ["c_api_quantized_mixed_group_fourbit.hip", "c_api_quantized_fourbit.hip"])
    single = {template_args(name, SINGLE): r for name, r in fourbit.items() if SINGLE in name}

    def counterpart(out, index, offset, n, weighted, source):
        prefix = "%s%s%sLi%sELb%sELNS0_11IndexSourceE%dE" % (out, index, offset, n, weighted, source)
        match = [r for a, r in single.items() if a.startswith(prefix)]
        assert len(match) == 1, prefix
        return match[0]

    lines, spills, below = [], 0, 0
    for name, r in sorted(mixed.items()):
        if MIXED not in name:
            continue
        args = template_args(name, MIXED)
        out, index, offset, n, weighted, staged = re.match(r"(f|DF16_)([il])([il])Li(\d+)ELb([01])ELb([01])", args).groups()
        others = [counterpart(out, index, offset, n, weighted, s) for s in ((0,) if staged == "1" else (1, 2))]
        spills += bool(r["ScratchSize"] or r["VGPRs Spill"] or r["SGPRs Spill"])
        lower = r["Occupancy"] < min(o["Occupancy"] for o in others)
        below += lower
        lines.append("%-4d %-4d %-7d %-6d %-6d %-5d %-3d | %-9s %-9s %s %s<%s>" % (
            r["VGPRs"], r["SGPRs"], r["ScratchSize"], r["VGPRs Spill"], r["SGPRs Spill"], r["LDS Size"], r["Occupancy"],
            " / ".join(str(o["VGPRs"]) for o in others), " / ".join(str(o["Occupancy"]) for o in others),
            "BELOW" if lower else "     ", KERNEL, args))
    print(__doc__.split("\n\n")[0])
    print("Template arguments as mangled: f / DF16_ = fp32 / fp16 output, i / l = int32 / int64 (IndexT, OffsetT), LiN = codes")
    print("per lane, first Lb0 / Lb1 = unweighted / weighted, second Lb0 / Lb1 = unstaged (CSR, or fixed hotness past the")
    print("staging budget) / staged in LDS.  Single-table columns: staged -> the LDS-staged instantiation; unstaged ->")
    print("cross-lane / global-load instantiation.  The single-table kernels of 16 and 8 codes per lane are compiled for")
    print("workgroups of up to 1,024 threads (at most 128 registers), those of 32 codes and the group's for 256.")
    print()
    print("%d instantiations; scratch or spills: %d; occupancy below the lowest single-table counterpart: %d, marked BELOW"
          % (len(lines), spills, below))
    print()
    print("4-bit quantized mixed group                       | single-table 4-bit")
    print("VGPR SGPR scratch Vspill Sspill LDS   occ | VGPR      occ             kernel")
    print("\n".join(lines))
    return 1 if spills else 0


if __name__ == "__main__":
    sys.exit(main())
