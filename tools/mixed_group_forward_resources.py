#!/usr/bin/env python3
"""Registers / scratch / occupancy of every mixed-width grouped forward kernel (GatherReduceMixedGroupKernel,
cuembed_amd/csrc/c_api_mixed_group.hip) next to the single-table instantiations of the same element, index and offset
types, lane width and weighting (GatherReduceKernel with fp32 accumulation in c_api_forward.hip), from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (as tools/grouped_forward_resources.py).  A staged instantiation has one
counterpart (indices staged in LDS); an unstaged one holds BOTH CSR walks -- the choice is made per workgroup at run time
-- so it is listed next to the cross-lane and the global-load instantiation.  No GPU needed; compiles two units.

    python tools/mixed_group_forward_resources.py > profiles/mixed_group_forward_resources.txt
"""
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grouped_forward_resources import SINGLE, remarks, template_args  # noqa: E402

MIXED = "28GatherReduceMixedGroupKernelI"


def main():
    with ThreadPoolExecutor(max_workers=2) as ex:
        mixed, forward = ex.map(remarks, ["c_api_mixed_group.hip", "c_api_forward.hip"])
    single = {template_args(name, SINGLE): r for name, r in forward.items() if SINGLE in name}

    def counterpart(elem, index, offset, n, weighted, source):
        prefix = "%sf%s%sLi%sELb%sELNS0_11IndexSourceE%dE" % (elem, index, offset, n, weighted, source)
        match = [r for a, r in single.items() if a.startswith(prefix)]
        assert len(match) == 1, prefix
        return match[0]

    lines, spills, below = [], 0, 0
    for name, r in sorted(mixed.items()):
        if MIXED not in name:
            continue
        args = template_args(name, MIXED)
        elem, index, offset, n, weighted, staged = re.match(r"(f|DF16_|DF16b)([il])([il])Li(\d+)ELb([01])ELb([01])E", args).groups()
        others = [counterpart(elem, index, offset, n, weighted, s) for s in ((0,) if staged == "1" else (1, 2))]
        spills += bool(r["ScratchSize"] or r["VGPRs Spill"] or r["SGPRs Spill"])
        lower = r["Occupancy"] < min(o["Occupancy"] for o in others)
        below += lower
        lines.append("%-4d %-4d %-7d %-6d %-6d %-5d %-3d | %-9s %-9s %s GatherReduceMixedGroupKernel<%s>" % (
            r["VGPRs"], r["SGPRs"], r["ScratchSize"], r["VGPRs Spill"], r["SGPRs Spill"], r["LDS Size"], r["Occupancy"],
            " / ".join(str(o["VGPRs"]) for o in others), " / ".join(str(o["Occupancy"]) for o in others),
            "BELOW" if lower else "     ", args))
    print(__doc__.split("\n\n")[0])
    print("Template arguments as mangled: f / DF16_ / DF16b = fp32 / fp16 / bf16, i / l = int32 / int64 (IndexT, OffsetT), LiN =")
    print("elements per lane, first Lb0 / Lb1 = unweighted / weighted, second Lb0 / Lb1 = unstaged (CSR, or fixed hotness")
    print("past the staging budget) / staged in LDS, Li8 = the unroll depth.  Single-table columns: staged -> the LDS-staged")
    print("instantiation; unstaged -> cross-lane / global-load instantiation.")
    print()
    print("%d instantiations; scratch or spills: %d; occupancy below the lowest single-table counterpart: %d, marked BELOW"
          % (len(lines), spills, below))
    print()
    print("mixed group                                       | single-table")
    print("VGPR SGPR scratch Vspill Sspill LDS   occ | VGPR      occ             kernel")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
