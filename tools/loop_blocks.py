"""Per basic block of a kernel's main loop: the copy, LDS, scalar and branch instructions.

Reads the listing of `make -C simplepathtracer_amd/csrc asm` (lib/obj/spt_kernels.s) and
nothing else.  The main loop is the outermost loop with the most blocks (render_body's
`for (;;)`, found from the compiler's loop comments); its blocks are printed in layout order with the loop depth the compiler's
block comments give, the count of v_mov (b32 / b64: the state copies where arms join and
on the back edge), ds_read / ds_write, SALU and branch instructions, the block's size and
where its branches go.  Blocks of inner loops (the walk, the sampler rounds: depth >= 2)
are summed into one line each unless --inner is given.

Usage: python tools/loop_blocks.py <kernel name fragment> [listing] [--inner] [--movs]
  e.g. python tools/loop_blocks.py render_kernelILb1ELi8EE
       python tools/loop_blocks.py render_kernel_svcILb1ELi8EE --movs   (prints the copies)
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTING = os.path.join(ROOT, "simplepathtracer_amd", "lib", "obj", "spt_kernels.s")


def kernel_lines(path, frag):
    """The lines of the first kernel whose symbol holds `frag`: (symbol, lines)."""
    sym, out = None, []
    with open(path) as f:
        for l in f:
            if sym is None:
                m = re.match(r"^(_Z\w+):", l)
                if m and frag in m.group(1):
                    sym = m.group(1)
                continue
            if l.startswith(".Lfunc_end"):
                break
            out.append(l.rstrip("\n"))
    if sym is None:
        sys.exit(f"no kernel with '{frag}' in {path}")
    return sym, out


def blocks_of(lines):
    """[(label, depth, [(op, operands)], outermost loop header)] in layout order, from the
    compiler's block comments (`in Loop: Header=BBn_m Depth=d`, `Parent Loop BBn_m Depth=1`,
    `This Loop Header: Depth=d`); the entry block is 'entry'."""
    raw, cur = [], ["entry", "", []]
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l)
        if m:
            raw.append(cur)
            cur = [m.group(1), m.group(2), []]
            continue
        if l.lstrip().startswith(";"):
            if not cur[2]:
                cur[1] += " " + l  # the loop comments go on after the label's line
            continue
        m = re.match(r"^\s+([a-z]\w+)\s*(.*?)\s*(;.*)?$", l)
        if m and not m.group(1).startswith("."):
            cur[2].append((m.group(1), m.group(2)))
    raw.append(cur)
    info = {}
    for label, note, _ in raw:
        me = label[2:]  # BBn_m
        d = re.search(r"Loop Header: Depth=(\d+)", note)
        top = re.search(r"Parent Loop (BB\d+_\d+) Depth=1\b", note)
        inl = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
        if d:
            info[me] = (int(d.group(1)), top.group(1) if top else me, None)
        elif inl:
            info[me] = (int(inl.group(2)), None, inl.group(1))
        else:
            info[me] = (0, None, None)
    blocks = []
    for label, _, ins in raw:
        depth, top, hdr = info.get(label[2:], (0, None, None))
        if hdr is not None:
            top = info.get(hdr, (0, None, None))[1]
        blocks.append((label, depth, ins, top))
    return blocks


def is_branch(op):
    return op.startswith(("s_cbranch", "s_branch"))


def is_salu(op):
    return op.startswith("s_") and not is_branch(op) and not op.startswith(
        ("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_memtime", "s_memrealtime"))


def counts(ins):
    c = dict(mov32=0, mov64=0, ds_read=0, ds_write=0, salu=0, branch=0, valu=0, n=len(ins))
    for op, _ in ins:
        if op.startswith("v_mov_b64") or op.startswith("v_pk_mov"):
            c["mov64"] += 1
        elif op.startswith("v_mov_b32") or op.startswith("v_accvgpr"):
            c["mov32"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_read"):
            c["ds_read"] += 1
        elif op.startswith("ds_write"):
            c["ds_write"] += 1
        elif is_branch(op):
            c["branch"] += 1
        elif is_salu(op):
            c["salu"] += 1
    return c


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        sys.exit(__doc__)
    inner, movs = "--inner" in sys.argv, "--movs" in sys.argv
    sym, lines = kernel_lines(args[1] if len(args) > 1 else LISTING, args[0])
    blocks = blocks_of(lines)
    # the main loop: the outermost loop with the most blocks (render_body's `for (;;)`); its
    # blocks need not be contiguous in the layout
    sizes = {}
    for b in blocks:
        if b[3]:
            sizes[b[3]] = sizes.get(b[3], 0) + 1
    if not sizes:
        sys.exit(f"{sym}: no loop")
    top = max(sizes, key=sizes.get)
    blocks = [b for b in blocks if b[3] == top]
    head, tail = 0, len(blocks) - 1
    print(f"{sym}: main loop .L{top}, {len(blocks)} blocks")
    base = min(b[1] for b in blocks[head:tail + 1])
    print(f"{'block':12s} {'depth':>5s} {'insts':>5s} {'valu':>5s} {'mov32':>5s} {'mov64':>5s} {'ds_rd':>5s} {'ds_wr':>5s} "
          f"{'salu':>5s} {'br':>3s}  branches to")
    keys = ("n", "valu", "mov32", "mov64", "ds_read", "ds_write", "salu", "branch")
    tot = dict.fromkeys(keys, 0)
    i = head
    while i <= tail:
        label, depth, ins, _ = blocks[i]
        j = i + 1
        if depth > base and not inner:
            # an inner loop: its blocks as one line
            ins = list(ins)
            while j <= tail and blocks[j][1] > base:
                ins += blocks[j][2]
                j += 1
            label += "+" + str(j - i - 1) if j - i > 1 else ""
        c = counts(ins)
        to = [a for op, a in ins if is_branch(op) and (depth == base or inner)]
        print(f"{label:12s} {depth - base + 1:5d} " + " ".join(f"{c[k]:5d}" for k in keys[:-1]) + f" {c['branch']:3d}  " + " ".join(to))
        if movs:
            for op, a in ins:
                if op.startswith(("v_mov_b", "v_pk_mov", "v_accvgpr")):
                    print(f"{'':14s}{op} {a}")
        for k in keys:
            tot[k] += c[k]
        i = j
    print(f"{'static total':12s} {'':5s} " + " ".join(f"{tot[k]:5d}" for k in keys[:-1]) + f" {tot['branch']:3d}")


if __name__ == "__main__":
    main()
