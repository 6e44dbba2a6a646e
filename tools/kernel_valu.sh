#!/bin/bash
# Static vector-instruction counts per kernel of one HIP source, from a device-only assembly build with the
# library's flags plus EXTRA: all VALU instructions (v_*), how many of them are lane moves
# (v_readlane_b32 / v_writelane_b32: scalar registers spilled into VGPR lanes -- they occupy the vector
# pipe, and kernel_regs.sh's scratch column does not show them; its SGPRs Spill column counts the registers,
# this the moves) and the s_nop hazard fillers.  Static counts: weigh them by trip counts before comparing kernels.
# usage: tools/kernel_valu.sh [csrc/file.hip | /abs/path/file.hip] [kernel name filter] [EXTRA flags]
SRC=${1:-csrc/shs_legacy.hip}
FLT=${2:-}
cd "$(dirname "$0")/../leisure-software-renderer_amd"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt \
  $3 --cuda-device-only -S -o - "$SRC" 2>/dev/null | python3 -c "
import sys, re
flt = sys.argv[1]
cur = None
rows = {}
for line in sys.stdin:
    m = re.match(r'^(_Z\w+):', line)
    if m:
        cur = m.group(1)
        rows[cur] = dict(valu=0, lane=0, nop=0)
        continue
    if cur is None: continue
    t = line.strip()
    op = t.split(None, 1)[0] if t else ''
    if op.startswith('v_'):
        rows[cur]['valu'] += 1
        if op in ('v_readlane_b32', 'v_writelane_b32'): rows[cur]['lane'] += 1
    elif op == 's_nop':
        rows[cur]['nop'] += 1
for k, r in rows.items():
    if flt in k and r['valu']:
        print(f\"{k[:70]:70s} VALU={r['valu']} lane_moves={r['lane']} s_nop={r['nop']}\")
" "$FLT"
