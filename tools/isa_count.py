"""Instruction-class histogram of one kernel (or of its hottest loop) in hipcc -S output.

usage: isa_count.py file.s mangled_substring [--loops] [--all] [--ops]
       isa_count.py file.s mangled_substring --cover [--all]
--all also prints the short blocks (with --cover: the loops that hold neither an MFMA nor a fragment wait); --ops adds the
opcode histogram of every printed block.
Counts VALU / MFMA / VMEM / LDS / SALU per basic block; with --loops prints every block that is a backward-branch target
(label .LBBx_y that some later s_cbranch jumps back to) — the loop bodies.

--cover audits how far ahead of their use the LDS fragment reads are issued.  LDS operations retire in order, so an
`s_waitcnt lgkmcnt(n)` retires every outstanding LDS operation but the youngest n.  For every such wait that retires at
least one ds_read, the wait's COVER is the number of MFMAs issued between the youngest read it retires and the wait itself:
the time the matrix pipe had work while that read was in flight.  Cover 0 means the wave issues a read and immediately
stalls on it.  Printed per loop (the blocks from a backward branch's target to the branch, in layout order; an inner loop
is walked once per pass of its outer loop) and for the kernel as a whole: the MFMA count and the histogram of covers.  A
loop is walked twice and the second pass is reported, so reads issued at the end of one iteration and waited on at the
top of the next are seen (the steady state).  Scalar memory loads share the counter and return out of order; they are
kept in the queue as non-reads, which can only lower a reported cover.
"""
import re, sys, collections

def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"): return "mfma"
    if op.startswith("v_cvt_pk_bf16") or op.startswith("v_cvt"): return "valu_cvt"
    if op.startswith("v_exp") or op.startswith("v_rcp") or op.startswith("v_log") or op.startswith("v_rsq") or op.startswith("v_sqrt"): return "valu_trans"
    if op.startswith("v_accvgpr"): return "valu_acc"
    if op.startswith("v_"): return "valu"
    if op.startswith("buffer_") or op.startswith("global_") or op.startswith("flat_") or op.startswith("scratch_"): return "vmem"
    if op.startswith("ds_"): return "lds"
    if op.startswith("s_waitcnt"): return "wait"
    if op.startswith("s_"): return "salu"
    return "other"

def kernel_body(lines, key):
    """The lines of the first function whose mangled name contains `key`, or None."""
    start = None
    for i, l in enumerate(lines):
        if l.startswith("_Z") and key in l and l.rstrip().endswith(":") is False and ":" in l:
            start = i; break
        if l.startswith("_Z") and key in l.split(":")[0]:
            start = i; break
    if start is None: return None
    end = start
    while end < len(lines) and not lines[end].startswith(".Lfunc_end"): end += 1
    return lines[start:end]

def full_blocks(body):
    """[(label, [instruction text])] in layout order; the first block is 'entry'."""
    blocks = []; cur = ("entry", [])
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append(cur); cur = (m.group(1), [])
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"): continue
        cur[1].append(t)
    blocks.append(cur)
    return blocks

def find_loops(blocks):
    """[(first block index, last block index)] per backward-branch target, widest extent, in layout order."""
    order = {b[0]: i for i, b in enumerate(blocks)}
    ext = {}
    for i, (name, ins) in enumerate(blocks):
        for t in ins:
            f = t.split()
            if (f[0].startswith("s_cbranch") or f[0] == "s_branch") and len(f) > 1 and order.get(f[1], 1 << 30) <= i:
                ext[order[f[1]]] = max(ext.get(order[f[1]], 0), i)
    return sorted(ext.items())

def walk_cover(instrs, passes=1):
    """(MFMAs per pass, covers of the last pass).  covers: one entry per s_waitcnt that retires a ds_read."""
    pending = []                     # outstanding lgkmcnt operations, oldest first: (is_read, MFMAs issued before it)
    mf = 0
    for k in range(passes):
        covers = []; mf0 = mf
        for t in instrs:
            op = t.split()[0]
            if op.startswith("v_mfma") or op.startswith("v_smfma"):
                mf += 1
            elif op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
                pending.append((op.startswith("ds_read") or op.startswith("ds_load"), mf))
            elif op == "s_waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", t)
                if not m: continue
                n = int(m.group(1))
                retired, pending = pending[:max(len(pending) - n, 0)], pending[max(len(pending) - n, 0):]
                reads = [at for is_read, at in retired if is_read]
                if reads: covers.append(mf - reads[-1])
    return mf - mf0, covers

def cover_report(lines, key):
    """[{'loop': header label or 'kernel', 'end': last block, 'mfma': n, 'covers': [...]}]; None if the kernel is missing."""
    body = kernel_body(lines, key)
    if body is None: return None
    blocks = full_blocks(body)
    flat = lambda a, b: [t for _, ins in blocks[a:b + 1] for t in ins]
    n, cov = walk_cover(flat(0, len(blocks) - 1))
    out = [dict(loop="kernel", end=blocks[-1][0], mfma=n, covers=cov)]
    for a, b in find_loops(blocks):
        n, cov = walk_cover(flat(a, b), passes=2)
        out.append(dict(loop=blocks[a][0], end=blocks[b][0], mfma=n, covers=cov))
    return out

def print_cover(rep):
    for r in rep:
        if not r["mfma"] and not r["covers"] and "--all" not in sys.argv: continue
        h = collections.Counter(r["covers"])
        hist = " · ".join(f"{c}: {h[c]}" for c in sorted(h)) or "-"
        least = min(r["covers"]) if r["covers"] else "-"
        print(f"{r['loop']:10s} ..{r['end']:10s} mfma={r['mfma']:5d} waits retiring ds_read={len(r['covers']):3d} "
              f"least cover={least}  cover: count  {hist}")

def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    if "--cover" in sys.argv:
        rep = cover_report(lines, key)
        if rep is None: sys.exit("kernel not found")
        print_cover(rep)
        return
    body = kernel_body(lines, key)
    if body is None: sys.exit("kernel not found")
    blocks = []; cur = ("entry", [])
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append(cur); cur = (m.group(1), [])
            continue
        t = l.strip()
        if not t or t.startswith(";") or t.startswith("."): continue
        cur[1].append(t.split()[0])
        if t.startswith("s_cbranch") or t.startswith("s_branch"):
            cur[1][-1] = t.split()[0] + " " + t.split()[1]
    blocks.append(cur)
    order = {b[0]: i for i, b in enumerate(blocks)}
    total = collections.Counter()
    for name, ops in blocks:
        c = collections.Counter(classify(o.split()[0]) for o in ops)
        total.update(c)
        back = [o.split()[1] for o in ops if o.startswith("s_cbranch") and len(o.split()) > 1 and order.get(o.split()[1], 1 << 30) <= order[name]]
        if "--loops" in sys.argv and not back: continue
        if len(ops) < 20 and "--all" not in sys.argv: continue
        print(f"{name:12s} n={len(ops):5d} back->{back} ", dict(c))
        if "--ops" in sys.argv:
            oc = collections.Counter(o.split()[0] for o in ops)
            print("   ", oc.most_common(40))
    print("TOTAL", dict(total))

if __name__ == "__main__":
    main()
