#!/usr/bin/env python3
"""Registers / scratch / occupancy of every mixed-width scatter-add kernel (MixedGroupScatterAddKernel,
cuembed_amd/csrc/c_api_mixed_group_backward.hip) next to the single-table instantiation of the same element and index
type, lane width, weighting and window depth (SegmentedScatterAddKernel in the reference order, c_api_backward.hip), and
of MixedGroupMeanScaleKernel next to GroupedMeanScaleKernel (c_api_grouped_backward.hip), from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (as tools/mixed_group_forward_resources.py).  No GPU needed; compiles three
units.

    python tools/mixed_group_backward_resources.py > profiles/mixed_group_backward_resources.txt
"""
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grouped_forward_resources import remarks, template_args  # noqa: E402

MIXED, SINGLE = "26MixedGroupScatterAddKernelI", "25SegmentedScatterAddKernelI"
MIXED_SCALE, GROUPED_SCALE = "25MixedGroupMeanScaleKernelI", "22GroupedMeanScaleKernelI"


def main():
    with ThreadPoolExecutor(max_workers=3) as ex:
        mixed, backward, grouped = ex.map(remarks, ["c_api_mixed_group_backward.hip", "c_api_backward.hip",
                                                    "c_api_grouped_backward.hip"])
    single = {template_args(name, SINGLE): r for name, r in backward.items() if SINGLE in name}
    scale = {template_args(name, GROUPED_SCALE): r for name, r in grouped.items() if GROUPED_SCALE in name}
    lines, spills, below = [], 0, 0
    for name, r in sorted(mixed.items()):
        if MIXED in name:
            args = template_args(name, MIXED)
            elem, index, n, weighted, window = re.match(r"(f|DF16_|DF16b)([il])Li(\d+)ELb([01])ELi(\d+)", args).groups()
            # (the reference order: kBlocked = false; the mangled list keeps the E that closes the last literal)
            other = single["%s%sLi%sELb%sELb0ELi%sE" % (elem, index, n, weighted, window)]
            kernel = "MixedGroupScatterAddKernel"
        elif MIXED_SCALE in name:
            args = template_args(name, MIXED_SCALE)
            other = scale[args]
            kernel = "MixedGroupMeanScaleKernel"
        else:
            continue
        spills += bool(r["ScratchSize"] or r["VGPRs Spill"] or r["SGPRs Spill"])
        lower = r["Occupancy"] < other["Occupancy"]
        below += lower
        lines.append("%-4d %-4d %-7d %-6d %-6d %-3d | %-4d %-3d %s %s<%s>" % (
            r["VGPRs"], r["SGPRs"], r["ScratchSize"], r["VGPRs Spill"], r["SGPRs Spill"], r["Occupancy"], other["VGPRs"],
            other["Occupancy"], "BELOW" if lower else "     ", kernel, args))
    print(__doc__.split("\n\n")[0])
    print("Template arguments as mangled: f / DF16_ / DF16b = fp32 / fp16 / bf16, i / l = int32 / int64 (IndexT; OffsetT for")
    print("the mean scale), LiN = elements per lane, Lb0 / Lb1 = unweighted / weighted, the last LiK of a scatter-add = the")
    print("depth of the rolling window (8: unsliced launches, 4: column-sliced ones).  LDS is dynamic (sized by the host).")
    print()
    print("%d instantiations; scratch or spills: %d; occupancy below the single-table counterpart: %d, marked BELOW"
          % (len(lines), spills, below))
    print()
    print("mixed group                              | single-table")
    print("VGPR SGPR scratch Vspill Sspill occ | VGPR occ       kernel")
    print("\n".join(lines))
    return 1 if spills else 0


if __name__ == "__main__":
    sys.exit(main())
