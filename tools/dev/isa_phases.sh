#!/bin/bash
# dev only: static instruction counts between the P2_TIMELINE stamps of the headline instantiation of the one-point fused kernel
# (armour_p2_eval_kernel<true, true, false, false, true, 6, true, 1, true, true>: g and jac, one point, d read, compact link x link normals, six slots, EX,
# one slicing round, no zero-normal test, one problem).
#   bash tools/dev/isa_phases.sh [CSRC]      CSRC: another checkout's armour_amd/csrc (default: this checkout's)
# Stretches are what lies between two stamps in the assembly, in file order (the collision path is laid out in program order); the first
# stamp is the kernel's entry stamp, the second P2_STAMP(0).  Also printed: the kernel's registers, scratch and occupancy.
set -eu
HERE=$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)
CSRC=${1:-$HERE/../../armour_amd/csrc}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
(cd "$CSRC" && "$HIPCC" -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DP2_TIMELINE -S --cuda-device-only p2_eval.hip -o "$TMP/p2_tl.s" 2>/dev/null)
python3 - "$TMP/p2_tl.s" <<'PY'
import re, sys
from collections import Counter
L = open(sys.argv[1]).read().split('\n')
HEAD = 'armour_p2_eval_kernelILb1ELb1ELb0ELb0ELb1ELi6ELb1ELi1ELb1ELb1EE'
a = next(i for i, l in enumerate(L) if l.startswith('_ZN') and ':' in l and HEAD in l.split(':')[0])
b = next(i for i in range(a, len(L)) if L[i].startswith('.Lfunc_end'))
K = L[a:b]
ins = lambda seg: [l.strip() for l in seg if l.startswith('\t') and not l.strip().startswith(('.', ';'))]
st = [i for i, l in enumerate(K) if 's_memrealtime' in l]
names = ['entry->0', '0->1', '1->2', '2->3', '3->4', '4->5', '5->6']
total = 0
for nme, (x, y) in zip(names, zip(st[:-1], st[1:])):
    seg = ins(K[x + 1:y])
    seg = [s for s in seg if not s.startswith('s_memrealtime')]
    c = Counter(s.split()[0].split('_')[0] for s in seg)
    op = Counter(s.split()[0] for s in seg)
    u64 = {k: v for k, v in op.items() if k in ('v_mad_u64_u32', 'v_lshl_add_u64', 'v_mul_lo_u32', 's_mul_i32', 's_mul_hi_i32', 's_mul_hi_u32', 's_addc_u32')}
    loads = sum(v for k, v in op.items() if re.match(r'(global|buffer|flat)_load|s_load|s_buffer_load', k))
    total += len(seg)
    print(f"{nme:9s} {len(seg):4d}  SALU {c['s']:3d} VALU {c['v']:3d} loads {loads:2d} (vector {sum(v for k, v in op.items() if re.match(r'(global|buffer|flat)_load', k)):2d})"
          f" LDS {c['ds']:2d} v_cndmask {sum(v for k, v in op.items() if k.startswith('v_cndmask')):3d} s_waitcnt {op['s_waitcnt']:2d} branches {sum(v for k, v in op.items() if 'branch' in k):2d}  {u64}")
print(f"collision path, stamp 0 -> 6: {total - len(ins(K[st[0] + 1:st[1]]))} instructions; whole kernel {len(ins(K))}")
# a fingerprint of the compiler's output for this kernel: the headline's speed has moved by 3 % with the instruction order alone
# (profiles/p2_vector_loads.txt), so compare this line before and after a toolchain change or an edit to any of the three roles
import hashlib
body = [re.sub(r'\.?LBB\d+_\d+', 'L', s) for s in ins(K) if not s.startswith('s_memrealtime')]
vloads = sum(1 for s in body if re.match(r'(global|buffer|flat)_load', s))
waits = [int(m.group(1)) for m in (re.search(r'vmcnt\((\d+)\)', s) for s in body if s.startswith('s_waitcnt')) if m]
print(f"fingerprint: vector loads {vloads}, s_waitcnt vmcnt {waits}, sha1 of the instruction stream {hashlib.sha1(chr(10).join(body).encode()).hexdigest()[:12]}")
tail = '\n'.join(L[b:b + 80])
for key in ('NumSgprs', 'NumVgprs', 'NumAgprs', 'ScratchSize', 'Occupancy', 'LDSByteSize'):
    m = re.search(r';\s*' + key + r':\s*(\d+)', tail)
    if m:
        print(f"{key} {m.group(1)}", end='   ')
print()
PY
