# Static instruction counts of the ImageIcp pixel loop (image_icp_head_kernel<true, false> by default, two pixels per trip) as the
# Makefile's flags compile it: VALU / SALU / memory instructions, s_nop, s_waitcnt's with their positions, VGPRs.  CPU only
# (hipcc -S).  The loop is the kernel's longest natural loop: from its header to the branch back to it; the rare
# wave-uniform slow paths that the compiler places behind that branch are not counted.
#   bash scripts/isa_loop_count.sh [extra hipcc flags]
#   KERNEL=<mangled name prefix> selects another kernel; KERNELS="a b c" counts several from one compilation
set -e
cd "$(dirname "$0")/.."
OUT=${TMPDIR:-/tmp}/a3d_isa && mkdir -p $OUT
#   ASM=<file> counts an assembly file made earlier (another commit's, say) instead of compiling
if [ -n "$ASM" ]; then cp "$ASM" $OUT/image_icp.s; else
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -w --offload-arch=gfx950 "$@" \
  -Iinclude -S --cuda-device-only align3d_amd/csrc/image_icp.hip -o $OUT/image_icp.s
fi
KERNEL=${KERNEL:-_ZN12_GLOBAL__N_121image_icp_head_kernelILb1ELb0ELb0EE}  # (KERNEL=_ZN12_GLOBAL__N_116image_icp_kernelILi1ELb0E: the last-block form)
python3 - $OUT/image_icp.s ${KERNELS:-$KERNEL} <<'PY'
import re, sys
s = open(sys.argv[1]).read().split('\n')
for name in sys.argv[2:]:
    starts = [i for i, l in enumerate(s) if re.match(re.escape(name) + r'\S*:', l)]
    if not starts:
        print(name, 'not found'); continue
    start = starts[0]
    end = next(i for i in range(start, len(s)) if s[i].startswith('.Lfunc_end'))
    k = s[start:end]
    best = None
    for i, l in enumerate(k):
        m = re.match(r'^(\.LBB\d+_\d+):.*Loop Header: Depth=1', l)
        if not m:
            continue
        back = [j for j in range(i, len(k)) if re.match(r'\s+s_c?branch\S*\s+' + re.escape(m.group(1)) + r'\s*$', k[j])]
        if back and (best is None or back[-1] - i > best[1] - best[0]):
            best = (i, back[-1])
    if best is None:
        print(name, 'no loop'); continue
    ops = [l.split() for l in k[best[0]:best[1] + 1] if l.startswith('\t') and not l.strip().startswith(('.', ';'))]
    n = lambda pred: sum(1 for o in ops if pred(o[0]))
    waits = ' '.join(f"{i}:{o[1]}" for i, o in enumerate(ops) if o[0] == 's_waitcnt' and 'vmcnt' in o[1])
    meta = ' '.join(l.strip('; \t') for l in s[end:end + 80] if any(x in l for x in ('; NumVgprs', '; Occupancy', '; ScratchSize')))
    print(f"{name}\n  per trip (2 pixels): ops {len(ops)} VALU {n(lambda o: o.startswith('v_'))} SALU {n(lambda o: o.startswith('s_'))} "
          f"(s_nop {n(lambda o: o == 's_nop')}, s_waitcnt {n(lambda o: o == 's_waitcnt')}) loads {n(lambda o: o.startswith(('global_load', 'ds_')))} "
          f"saveexec {n(lambda o: 'saveexec' in o)} | {meta}\n  vmcnt waits (index in loop): {waits}")
    open(sys.argv[1].replace('.s', '.' + re.sub(r'\W', '_', name) + '.loop.s'), 'w').write('\n'.join(k[best[0]:best[1] + 1]))
PY
