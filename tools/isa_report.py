#!/usr/bin/env python3
"""Static instruction mix and resources of every kernel in a gfx950 assembly file (python st-nerf_amd/build.py --asm SOURCE OUT):
vector / scalar / LDS / memory instruction counts, v_readlane / v_writelane (SGPR spills into VGPR lanes show up here),
registers, scratch, occupancy.   python tools/isa_report.py file.s [name filter]"""
import collections
import sys

import asm_listing

flt = sys.argv[2] if len(sys.argv) > 2 else ""
for name, k in asm_listing.kernels(open(sys.argv[1]).read()).items():
    if flt not in name:
        continue
    c = collections.Counter()
    for l in k["body"].split('\n'):
        s = l.strip()
        if not s or s.startswith(';') or s.startswith('.'):
            continue
        op = s.split()[0]
        if op.endswith(':'):
            continue
        kind = 'valu' if op.startswith('v_') else 'salu' if op.startswith('s_') else 'lds' if op.startswith('ds_') else 'vmem' if op.startswith(('global_', 'buffer_', 'scratch_')) else 'other'
        c[kind] += 1
        if op in ('v_readlane_b32', 'v_writelane_b32'):
            c['lane_rw'] += 1
        if op == 's_waitcnt':
            c['waitcnt'] += 1
    print(name[:70], dict(c), 'vgpr', k['NumVgprs'], 'sgpr', k['TotalNumSgprs'], 'scratch', k['ScratchSize'], 'occupancy', k['Occupancy'])
