"""Basic blocks of one loop of a kernel and the lane moves on a path through it.

    python tools/isa_hot_path.py /tmp/rk.s 'k_gossip_fusedILb0ELi3ELi0ELb0ELb0E' \\
           [--loop FIRST,LAST] [--copy 2 --from-src 1972 --to-src 2133] \\
           [--skip-src 2020-2053,device_util.h:220-238] [--sum 3,4,9] [--quiet]

The listing is the `-gline-tables-only` build's `llvm-objdump -d -l` output (recipe in
tools/isa_lines.py).  The loop is given by the instruction indices `isa_lines.py` prints for it;
without `--loop` the kernel's outermost loop (the longest backward branch) is taken.  It is split
into basic blocks (a block starts at every branch target and behind every branch), and per block
the tool prints its VALU count, the lane reads and lane writes of the SGPR-spill registers
(`v_readlane_b32` from / `v_writelane_b32` into a VGPR that the kernel writes lanes of; the
kernel's own readlanes of data registers are listed apart), its vector memory operations (`mem`;
scalar loads count as SALU, `ds_*` as LDS, as in isa_lines.py), where it branches and its source
lines.

An unrolled loop holds several copies of its body.  `--copy N --from-src A --to-src B` keeps the
N-th run of blocks that starts at a block holding source line A and ends at the next block
holding line B (lines without a file name are relay_kernels.hip's).

A path is a set of blocks: those named with `--sum`, or every block left after `--skip-src` drops
the blocks that hold an instruction of the given source-line ranges (the code a narrow peer does
not run: the per-task code, the wide-row chunk loops, the wide pass, the windowed list loop, the
row-by-row flush).  A block on the path counts once, the body of an inner loop included, so the
sum is the fixed work of one visit, not its trip counts.

Limits.  The sum is static: both sides of a branch whose blocks are all on the path are added,
although a visit runs one of them, so it is an upper count of the straight-line work and not what
one visit executes; compare two builds of the same source with it, not a build with a hand walk.
The `--skip-src` ranges are line numbers of one tree: a tree whose lines moved needs its own
ranges for the same statements (the header of each committed listing states the ranges used).
"""
import argparse
import collections
import re

from isa_lines import kind

MAIN = "relay_kernels.hip"


def load(path, kernel):
    """[(address, opcode, operands, branch target, 'file:line')] of one kernel."""
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^[0-9a-f]+ <.*" + kernel, l))
    base = int(lines[start].split()[0], 16)
    ins, src = [], None
    for l in lines[start + 1:]:
        if re.match(r"^[0-9a-f]+ <", l):
            break
        m = re.match(r"^; (\S+):(\d+)", l)
        if m:
            src = (m.group(1).split("/")[-1], int(m.group(2)))
            continue
        m = re.match(r"^\t(\S+)(.*?)//\s*([0-9A-Fa-f]+):", l)
        if m:
            t = re.search(r"\+0x([0-9a-f]+)>", l)
            ins.append((int(m.group(3), 16), m.group(1), m.group(2).strip(),
                        base + int(t.group(1), 16) if t else None, src))
    return ins


def is_branch(op):
    return op.startswith("s_cbranch") or op == "s_branch"


def outer_loop(ins):
    idx = {x[0]: i for i, x in enumerate(ins)}
    best = None
    for i, (a, op, _, tgt, _) in enumerate(ins):
        if is_branch(op) and tgt is not None and tgt <= a and tgt in idx:
            if best is None or i - idx[tgt] > best[1] - best[0]:
                best = (idx[tgt], i)
    return best


def blocks(ins, first, last):
    idx = {x[0]: i for i, x in enumerate(ins)}
    leaders = {first}
    for i in range(first, last + 1):
        _, op, _, tgt, _ = ins[i]
        if is_branch(op):
            if i + 1 <= last:
                leaders.add(i + 1)
            if tgt in idx and first <= idx[tgt] <= last:
                leaders.add(idx[tgt])
    order = sorted(leaders)
    return [(b, (order[n + 1] - 1) if n + 1 < len(order) else last) for n, b in enumerate(order)]


def src_point(text):
    f, _, l = text.rpartition(":")
    return (f or MAIN, int(l))


def src_ranges(text):
    out = []
    for part in filter(None, (text or "").split(",")):
        f, _, r = part.rpartition(":")
        lo, _, hi = r.partition("-")
        out.append((f or MAIN, int(lo), int(hi or lo)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--loop", help="FIRST,LAST instruction indices (isa_lines.py prints them)")
    ap.add_argument("--copy", type=int, help="the N-th copy of an unrolled body (from 1)")
    ap.add_argument("--from-src", help="source line of a copy's first block")
    ap.add_argument("--to-src", help="source line of a copy's last block")
    ap.add_argument("--skip-src", help="source-line ranges whose blocks are off the path")
    ap.add_argument("--sum", help="block numbers on the path")
    ap.add_argument("--quiet", action="store_true", help="the sums only")
    a = ap.parse_args()
    ins = load(a.listing, a.kernel)
    spill = {args.split(",")[0].strip() for _, op, args, _, _ in ins if op == "v_writelane_b32"}
    first, last = map(int, a.loop.split(",")) if a.loop else outer_loop(ins)
    idx = {x[0]: i for i, x in enumerate(ins)}
    bl = blocks(ins, first, last)
    srcs = [collections.Counter(ins[i][4] for i in range(b, e + 1) if ins[i][4]) for b, e in bl]
    keep = range(len(bl))
    if a.copy:
        lo_pt, hi_pt = src_point(a.from_src), src_point(a.to_src)
        n, found = 0, 0
        while n < len(bl):
            if lo_pt in srcs[n]:
                end = next((m for m in range(n + 1, len(bl)) if hi_pt in srcs[m]), None)
                if end is None:
                    break
                found += 1
                if found == a.copy:
                    keep = range(n, end + 1)
                    break
                n = end
            n += 1
        if found != a.copy:
            raise SystemExit(f"copy {a.copy} not found ({found} copies)")
    skip = src_ranges(a.skip_src)
    named = {int(x) for x in a.sum.split(",")} if a.sum else None
    print(f"kernel {a.kernel}: {len(ins)} instructions, loop [{first}, {last}], {len(bl)} blocks, "
          f"blocks B{keep[0]}..B{keep[-1]} shown, SGPR-spill registers {sorted(spill)}")
    tot = collections.Counter()
    for n in keep:
        b, e = bl[n]
        c = collections.Counter()
        for i in range(b, e + 1):
            _, op, args, _, _ = ins[i]
            c[kind(op)] += 1
            if op == "v_readlane_b32":
                reg = args.split(",")[1].strip() if "," in args else ""
                c["rd" if reg in spill else "rd_data"] += 1
            elif op == "v_writelane_b32":
                c["wr"] += 1
        off = any(f == sf and lo <= ln <= hi for (f, ln) in srcs[n] for sf, lo, hi in skip)
        on = (n in named) if named is not None else not off
        _, op, _, tgt, _ = ins[e]
        to = ""
        if is_branch(op) and tgt is not None:
            t = idx.get(tgt)
            tb = next((m for m, (bb, ee) in enumerate(bl) if t is not None and bb <= t <= ee), None)
            to = f" {op}->{'B%d' % tb if tb is not None else 'out'}"
        if on:
            tot.update(c)
            tot["blocks"] += 1
        if not a.quiet:
            ls = " ".join(f"{l}" if f == MAIN else f"{f}:{l}" for f, l in sorted(srcs[n]))
            print(f"{'*' if on else ' '} B{n} [{b}, {e}] VALU {c['v']} lane reads {c['rd']} lane writes {c['wr']} "
                  f"data readlanes {c['rd_data']} SALU {c['s']} mem {c['mem']} LDS {c['ds']}{to} | {ls}")
    print(f"path: {tot['blocks']} blocks, VALU {tot['v']}, lane reads {tot['rd']}, lane writes {tot['wr']}, "
          f"lane moves {tot['rd'] + tot['wr']}, data readlanes {tot['rd_data']}, SALU {tot['s']}, "
          f"mem {tot['mem']}, LDS {tot['ds']}")


if __name__ == "__main__":
    main()
