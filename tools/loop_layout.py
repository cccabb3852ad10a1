#!/usr/bin/env python3
"""Where the 8-byte instructions of a kernel's loops start.

    python tools/loop_layout.py f32 8 [--kernel NAME] [--depth 3] [-v]      build the unit as tools/isa.py does, assemble, disassemble
    llvm-objdump -d code_object | python tools/loop_layout.py - [--kernel NAME] [--depth 3]

One wave per SIMD has nothing to hide its instruction fetch behind: an 8-byte instruction that starts at 4 mod 8 costs it up to a
cycle more than one that starts at 0 mod 8 (tools/valu_ops_rate.hip, profiles/r13_loop_layout.txt).  For every loop of the named
kernel at the given depth this reports the loop's size in bytes, how many 8-byte and 4-byte instructions it holds and the 8-byte ones
at 4 mod 8, each with its line.  Loops are the natural loops of the control-flow graph read from the branches; the depth of a loop is the
number of loops around it, itself included (the leapfrog loop of k_chain lies in the thinning loop in the iteration loop: 3).
The default kernel is the headline one, k_chain<float, 8, 16, reg, 13, HMC>.
"""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HEADLINE = "_ZN2lr7k_chainIfLi8ELi16ELi0ELi13ELi2EEE"  # k_chain<float, 8, 16, MODE_REG, 13, KIND_HMC>: prefix of the mangled name

_SYM = re.compile(r"^[0-9a-fA-F]+ <([^>]+)>:\s*$")
_INS = re.compile(r"^\s+(\S+)(.*?)//\s*([0-9A-Fa-f]+):((?:\s+[0-9A-Fa-f]{8})+)")


def parse_listing(text):
    """llvm-objdump -d text -> {symbol: [(address, bytes, mnemonic, words, line)]}, in listing order"""
    kernels, cur = {}, None
    for line in text.split("\n"):
        m = _SYM.match(line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        m = _INS.match(line)
        if m and cur is not None:
            words = [int(w, 16) for w in m.group(4).split()]
            cur.append((int(m.group(3), 16), 4 * len(words), m.group(1), words, line.strip()))
    return kernels


def _target(addr, words):
    simm = words[0] & 0xFFFF
    return addr + 4 + 4 * (simm - 0x10000 if simm & 0x8000 else simm)


def loops(instrs):
    """Natural loops of a kernel's control-flow graph -> [(sorted instruction indices, depth)], ordered by header address; depth 1 =
    outermost.  Basic blocks from the branch instructions, dominators (Cooper / Harvey / Kennedy), one loop per header that is the
    target of an edge from a block it dominates; the depth of a loop is the number of loops that contain its header."""
    index = {ins[0]: k for k, ins in enumerate(instrs)}
    n = len(instrs)
    leaders = {0}
    for k, (addr, _, mnem, words, _) in enumerate(instrs):
        if mnem.startswith(("s_cbranch_", "s_branch")):
            t = index.get(_target(addr, words))
            if t is not None:
                leaders.add(t)
            leaders.add(k + 1)
        elif mnem.startswith(("s_endpgm", "s_setpc", "s_swappc")):
            leaders.add(k + 1)
    starts = sorted(x for x in leaders if x < n)
    block_of = {s: b for b, s in enumerate(starts)}
    ends = starts[1:] + [n]
    succ = []
    for s, e in zip(starts, ends):
        addr, _, mnem, words, _ = instrs[e - 1]
        out = []
        if mnem.startswith(("s_cbranch_", "s_branch")):
            t = index.get(_target(addr, words))
            if t is not None:
                out.append(block_of[t])
        if not mnem.startswith(("s_branch", "s_endpgm", "s_setpc")) and e < n:
            out.append(block_of[e])
        succ.append(out)
    nb = len(starts)
    pred = [[] for _ in range(nb)]
    for b, out in enumerate(succ):
        for t in out:
            pred[t].append(b)
    order, seen, stack = [], {0}, [(0, iter(succ[0]))]  # post-order from the entry block
    while stack:
        b, it = stack[-1]
        for t in it:
            if t not in seen:
                seen.add(t)
                stack.append((t, iter(succ[t])))
                break
        else:
            order.append(b)
            stack.pop()
    rank = {b: k for k, b in enumerate(order)}
    idom = {0: 0}
    changed = True
    while changed:
        changed = False
        for b in reversed(order[:-1]):
            new = None
            for q in pred[b]:
                if q in idom:
                    if new is None:
                        new = q
                    else:
                        x, y = q, new
                        while x != y:
                            while rank[x] < rank[y]:
                                x = idom[x]
                            while rank[y] < rank[x]:
                                y = idom[y]
                        new = x
            if idom.get(b) != new:
                idom[b] = new
                changed = True

    def dominates(h, b):
        while b != h and b != 0:
            b = idom[b]
        return b == h

    bodies = {}
    for b in order:
        for h in succ[b]:
            if h in idom and dominates(h, b):  # a back edge b -> h
                body = bodies.setdefault(h, {h})
                work = [b]
                while work:
                    x = work.pop()
                    if x not in body:
                        body.add(x)
                        work.extend(q for q in pred[x] if q in idom)
    res = []
    for h in sorted(bodies):
        depth = sum(1 for body in bodies.values() if h in body)
        res.append((sorted(k for b in bodies[h] for k in range(starts[b], ends[b])), depth))
    return res


def loop_report(instrs, members):
    """Counts for the instructions of one loop (`members`: indices): size in bytes, whether the loop is one contiguous run, 8-byte
    and 4-byte instructions, others, the 8-byte ones that start at 4 mod 8 as (address, line), and every instruction as (mnemonic, bytes)."""
    body = [instrs[k] for k in members]
    return {"first": body[0][0], "bytes": sum(i[1] for i in body), "instructions": len(body),
            "contiguous": members == list(range(members[0], members[0] + len(members))),
            "n8": sum(1 for i in body if i[1] == 8), "n4": sum(1 for i in body if i[1] == 4),
            "other": sum(1 for i in body if i[1] not in (4, 8)),
            "straddling": [(i[0], i[4]) for i in body if i[1] == 8 and i[0] % 8 == 4],
            "tail": [i[2] for i in body[-3:]], "sizes": [(i[2], i[1]) for i in body]}


def kernel_loops(text, kernel=HEADLINE, depth=3):
    """-> (symbol, [loop_report of every loop of that depth]) of the one kernel whose mangled name contains `kernel`"""
    kernels = parse_listing(text)
    names = [k for k in kernels if kernel in k]
    if len(names) != 1:
        raise LookupError(f"{len(names)} kernels match {kernel!r}" + (": " + ", ".join(names[:4]) if names else f" among {len(kernels)}"))
    instrs = kernels[names[0]]
    return names[0], [loop_report(instrs, members) for members, d in loops(instrs) if d == depth]


def unit_disassembly(dt="f32", p=8):
    """Disassembly of one instantiation unit's gfx950 code object: the object file of the built library when it is current, else the
    unit compiled for the device alone with the library's flags (no GPU needed)."""
    from logreg_amd import build as B
    from logreg_amd.isa_gate import llvm_tool
    objdump = llvm_tool("llvm-objdump")
    obj = os.path.join(B.OBJDIR, f"lr_inst_{dt}_p{p}.o")
    with tempfile.TemporaryDirectory(prefix="lr_layout_") as tmp:
        if os.path.exists(obj) and not B.needs_build() and not B.built_extra():
            link = os.path.join(tmp, "unit.o")
            os.symlink(obj, link)
            subprocess.run([objdump, "--offloading", link], capture_output=True, text=True, check=True)  # writes <link>.N.<target>
            cos = [os.path.join(tmp, f) for f in os.listdir(tmp) if f.startswith("unit.o.") and f.endswith(B.ARCH)]
            co = cos[0]
        else:
            co = os.path.join(tmp, "unit.co")
            wide = p > 32
            defs = [f"-DLR_P={p}", f"-DLR_SFX={dt}_p{p}", f"-DLR_DTYPE={0 if dt == 'f32' else 1}"]
            if not wide:
                defs.append(f"-DLR_T={'float' if dt == 'f32' else 'double'}")
            subprocess.run([B._hipcc(), *B.COMMON, *defs, os.path.join(B.CSRC, "lr_inst_wide.hip" if wide else "lr_inst.hip"),
                            "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", co], check=True)  # (an ELF, not an offload bundle)
        return subprocess.run([objdump, "-d", co], capture_output=True, text=True, check=True).stdout


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("unit", nargs="+", help="'-' (a disassembly listing on stdin) or: f32|f64 and the padded p")
    ap.add_argument("--kernel", default=HEADLINE, help="part of the kernel's mangled name")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("-v", action="store_true", help="list the straddling instructions")
    a = ap.parse_args(argv)
    text = sys.stdin.read() if a.unit == ["-"] else unit_disassembly(a.unit[0], int(a.unit[1]))
    name, reports = kernel_loops(text, a.kernel, a.depth)
    print(f"{name}: {len(reports)} loops at depth {a.depth}")
    for r in reports:
        print(f"loop at {r['first']:#x} ({r['first'] % 64} mod 64): {r['bytes']} bytes{'' if r['contiguous'] else ' (not contiguous)'}, {r['instructions']} instructions: {r['n8']} of 8 bytes, "
              f"{r['n4']} of 4, {r['other']} other; {len(r['straddling'])} of 8 bytes start at 4 mod 8; ends with {' / '.join(r['tail'])}")
        by = {}
        for _, line in r["straddling"]:
            by[line.split()[0]] = by.get(line.split()[0], 0) + 1
        if by:
            print("  at 4 mod 8: " + ", ".join(f"{n} {k}" for k, n in sorted(by.items())))
        if a.v:
            for addr, line in r["straddling"]:
                print(f"  {addr:#x}: {line}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
