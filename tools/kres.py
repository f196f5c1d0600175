#!/usr/bin/env python3
"""Per-kernel resource table of one .hip source (hipcc -Rpass-analysis=kernel-resource-usage): VGPRs, AGPRs, spills, scratch,
LDS, occupancy.  usage: tools/kres.py csrc/attn.hip [name-filter]      (the compile and the parser are kres_diff.py's)"""
import sys
from kres_diff import RES, kernels

flt = sys.argv[2] if len(sys.argv) > 2 else ""
print(f"{'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'vspill':>6} {'sspill':>6} {'scratch':>8} {'LDS':>7} {'occ':>4}  kernel")
for name, (res, _) in sorted(kernels(sys.argv[1], None).items()):
    if flt in name:
        v = [res.get(key, "?") for _, key in RES]
        print(f"{v[0]:>5} {v[1]:>5} {v[2]:>5} {v[3]:>6} {v[4]:>6} {v[5]:>8} {v[6]:>7} {v[7]:>4}  {name}")
