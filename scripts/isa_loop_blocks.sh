# What scripts/isa_loop_count.sh leaves out: the wave-uniform slow-path blocks that the compiler places behind the pixel
# loop's back branch (the IEEE-divide fallback of stage B, the shifted intensity samples of stage D and their request).
# For each kernel: the loop found the same way, then every block outside it that is entered from the loop and returns to
# it, with its instruction counts, its loads and every s_waitcnt vmcnt in it; and the vmcnt waits of the loop itself.
# CPU only (hipcc -S).
#   bash scripts/isa_loop_blocks.sh [extra hipcc flags]
#   KERNELS="a b c" (mangled name prefixes) selects the kernels; ASM=<file> reads an assembly file made earlier
set -e
cd "$(dirname "$0")/.."
OUT=${TMPDIR:-/tmp}/a3d_isa && mkdir -p $OUT
if [ -n "$ASM" ]; then cp "$ASM" $OUT/image_icp.s; else
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -w --offload-arch=gfx950 "$@" \
  -Iinclude -S --cuda-device-only align3d_amd/csrc/image_icp.hip -o $OUT/image_icp.s
fi
K=_ZN12_GLOBAL__N_121image_icp_head_kernelI
KERNELS=${KERNELS:-"${K}Lb1ELb1ELb0ELb1ELb0EE ${K}Lb1ELb1ELb0ELb0ELb0EE ${K}Lb1ELb0ELb0ELb0ELb0EE ${K}Lb0ELb0ELb0ELb0ELb0EE"}
python3 - $OUT/image_icp.s $KERNELS <<'PY'
import re, sys
s = open(sys.argv[1]).read().split('\n')
LABEL = re.compile(r'^(\.LBB\d+_\d+):')
BRANCH = re.compile(r'\s+(s_c?branch\S*)\s+(\.LBB\d+_\d+)\s*$')
is_op = lambda l: l.startswith('\t') and not l.strip().startswith(('.', ';'))
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
    # labelled blocks of the kernel: [label, first line, last line + 1]
    at = [(LABEL.match(l).group(1), i) for i, l in enumerate(k) if LABEL.match(l)]
    blocks = {lab: (i, at[n + 1][1] if n + 1 < len(at) else len(k)) for n, (lab, i) in enumerate(at)}
    order = [lab for lab, _ in at]
    in_loop = lambda lab: best[0] <= blocks[lab][0] <= best[1]

    def succ(lab):
        a, b = blocks[lab]
        out = [BRANCH.match(l).group(2) for l in k[a:b] if BRANCH.match(l)]
        ops = [l.split()[0] for l in k[a:b] if is_op(l)]
        if not ops or ops[-1] not in ('s_branch', 's_endpgm'):
            n = order.index(lab) + 1
            if n < len(order):
                out.append(order[n])
        return out

    def reach(seeds, edges):
        seen, todo = set(), list(seeds)
        while todo:
            x = todo.pop()
            if x in seen or in_loop(x):
                continue
            seen.add(x)
            todo += edges(x)
        return seen

    pred = {}
    for lab in order:
        for t in succ(lab):
            pred.setdefault(t, []).append(lab)
    loop_labels = [lab for lab in order if in_loop(lab)]
    entered = reach([t for lab in loop_labels for t in succ(lab)], succ)
    returning = reach([p for lab in loop_labels for p in pred.get(lab, [])], lambda x: pred.get(x, []))
    slow = [lab for lab in order if lab in entered and lab in returning]
    loop_ops = [l.split() for l in k[best[0]:best[1] + 1] if is_op(l)]
    lw = [o[1] for o in loop_ops if o[0] == 's_waitcnt' and 'vmcnt' in o[1]]
    print(f"{name}\n  loop: ops {len(loop_ops)}, vmcnt waits {len(lw)}, of them vmcnt(0): {sum(1 for w in lw if w.startswith('vmcnt(0)'))}")
    tot = {'ops': 0, 'valu': 0, 'loads': 0, 'waits': 0, 'drains': 0}
    for lab in slow:
        a, b = blocks[lab]
        ops = [l.split() for l in k[a:b] if is_op(l)]
        waits = [o[1] for o in ops if o[0] == 's_waitcnt' and 'vmcnt' in o[1]]
        loads = [o[0] for o in ops if o[0].startswith('global_load')]
        back_to = [t for t in succ(lab) if in_loop(t)]
        print(f"  {lab}: ops {len(ops)} VALU {sum(1 for o in ops if o[0].startswith('v_'))} loads {len(loads)} "
              f"({' '.join(sorted(set(loads)))}) vmcnt waits [{' '.join(waits)}] -> {' '.join(back_to) or '(next block)'}")
        tot['ops'] += len(ops); tot['valu'] += sum(1 for o in ops if o[0].startswith('v_')); tot['loads'] += len(loads)
        tot['waits'] += len(waits); tot['drains'] += sum(1 for w in waits if w.startswith('vmcnt(0)'))
    print(f"  slow-path blocks {len(slow)}: ops {tot['ops']} VALU {tot['valu']} loads {tot['loads']} vmcnt waits {tot['waits']}, "
          f"of them vmcnt(0): {tot['drains']}")
PY
