"""Development tool: static vector-instruction counts of one kernel of a tools/disasm.py listing.
    python tools/disasm.py 10 15 0 8192 186 > out.s && python tools/static_count.py out.s [kernel]
Prints the v_* instructions of the kernel (default crbm_gibbs_sparse_geo) per region, the listing split at s_barrier
(profiles/diet_static.txt: prologue, state load + table copy, v|h, h|v + tail), a histogram of the mnemonics of the
h|v region, and the h|v main path: the straight-line run that holds the region's v_exp_f32, from the last branch
target in front of the first one to the first branch behind the last one (the head of the item loop to the test that
enters the exact path).  A static count: every loop body is counted once."""
import collections
import re
import sys

path = sys.argv[1]
kernel = sys.argv[2] if len(sys.argv) > 2 else "crbm_gibbs_sparse_geo"
body, inside = [], False
for line in open(path):
    m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
    if m:
        inside = m.group(1) == kernel
        continue
    if inside and line.strip():
        body.append(line.strip())
if not body:
    sys.exit("no kernel %s in %s" % (kernel, path))
# an instruction line is "mnemonic operands // ADDRESS: encoding [<kernel+0xOFFSET>]"; the listing has no labels, a
# branch names its target by offset from the kernel's first instruction
rows, targets, base = [], set(), None
for t in body:
    m = re.search(r"//\s*([0-9A-Fa-f]+):", t)
    addr = int(m.group(1), 16) if m else None
    if base is None and addr is not None:
        base = addr
    mn = t.split()[0]
    if mn.startswith("s_cbranch") or mn == "s_branch":
        b = re.search(r"<%s\+0x([0-9a-f]+)>" % re.escape(kernel), t)
        targets.add(int(b.group(1), 16) if b else 0)
    rows.append((mn, t, addr))
ins = [(mn, t, addr is not None and addr - base in targets) for mn, t, addr in rows]   # (mnemonic, text, is a branch target)
regions, cur = [], []
for mn, t, lab in ins:
    cur.append((mn, t, lab))
    if mn == "s_barrier":
        regions.append(cur)
        cur = []
regions.append(cur)
counts = [sum(1 for mn, _, _ in r if mn.startswith("v_")) for r in regions]
print("%s: %d regions split at s_barrier, vector instructions %s, total %d" % (kernel, len(regions), counts, sum(counts)))
# the region with the most v_exp_f32 behind the first one that has any is h|v (v|h holds 16, h|v ten at K = 10)
with_exp = [i for i, r in enumerate(regions) if any(mn.startswith("v_exp_f32") for mn, _, _ in r)]
hv = regions[with_exp[-1]]
hist = collections.Counter(mn for mn, _, _ in hv if mn.startswith("v_"))
print("h|v region mnemonics:", ", ".join("%s %d" % kv for kv in sorted(hist.items(), key=lambda kv: -kv[1])))
exps = [i for i, (mn, _, _) in enumerate(hv) if mn.startswith("v_exp_f32")]
first, last = exps[0], exps[-1]
is_branch = lambda mn: mn.startswith("s_cbranch") or mn == "s_branch"
lo = first
while lo > 0 and not hv[lo][2] and not is_branch(hv[lo - 1][0]):
    lo -= 1
hi = last
while hi + 1 < len(hv) and not hv[hi + 1][2] and not is_branch(hv[hi + 1][0]):
    hi += 1
run = hv[lo:hi + 1]
rh = collections.Counter(mn for mn, _, _ in run if mn.startswith("v_"))
print("h|v main path: %d vector instructions (%d v_exp_f32 in it of %d in the region)" % (sum(rh.values()), sum(n for k, n in rh.items() if k.startswith("v_exp_f32")), len(exps)))
print("  ", ", ".join("%s %d" % kv for kv in sorted(rh.items(), key=lambda kv: -kv[1])))
