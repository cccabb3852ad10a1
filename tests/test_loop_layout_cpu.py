"""tools/loop_layout.py counts what it says it counts, and the headline kernel's leapfrog loop keeps the layout that
profiles/r13_loop_layout.txt paid for: no 8-byte instruction of the loop starts at 4 mod 8 (one wave per SIMD pays up to a cycle for each
that does), in no more than 174 instructions.  Cross-compiled: no GPU needed."""
import os
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import loop_layout  # noqa: E402


def listing(sizes, head=0x100):
    """An llvm-objdump -d listing of one kernel: a prologue, ONE loop of instructions of the given sizes (4: v_exp_f32_e32, 8: v_pk_fma_f32)
    closed by s_cmp_lg_u32 / s_cbranch_scc1 back to its head, s_endpgm."""
    lines = ["", "Disassembly of section .text:", "", "0000000000000000 <kern>:"]
    addr = 0

    def emit(text, words):
        nonlocal addr
        lines.append(f"\t{text:<60}// {addr:012X}: " + " ".join(f"{w:08X}" for w in words))
        addr += 4 * len(words)

    while addr < head:
        emit("s_nop 0", [0xBF800000])
    for s in sizes:
        if s == 8:
            emit("v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[0:1]", [0xD3B04000, 0x1C020902])
        else:
            emit("v_exp_f32_e32 v6, v6", [0x7E0C4106])
    emit("s_cmp_lg_u32 s0, 0", [0xBF078000])
    back = (head - (addr + 4)) // 4
    emit(f"s_cbranch_scc1 {back & 0xFFFF}", [0xBF850000 | (back & 0xFFFF)])
    emit("s_endpgm", [0xBF810000])
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("sizes,n8,n4,straddling", [
    ([8, 8, 8, 8, 8, 8], 6, 2, 0),              # all aligned (the two 4-byte ones are the loop control)
    ([4, 8, 8, 8, 8, 8], 5, 3, 5),              # one 4-byte instruction in front of five 8-byte ones
    ([8, 8, 4, 4, 8, 8, 8], 5, 4, 0),           # a pair of 4-byte instructions in the middle
])
def test_counter_on_hand_written_listings(sizes, n8, n4, straddling):
    name, reports = loop_layout.kernel_loops(listing(sizes), "kern", depth=1)
    assert name == "kern" and len(reports) == 1
    r = reports[0]
    assert (r["first"], r["contiguous"]) == (0x100, True)
    assert (r["n8"], r["n4"], r["other"]) == (n8, n4, 0)
    assert r["instructions"] == len(sizes) + 2 and r["bytes"] == sum(sizes) + 8
    assert len(r["straddling"]) == straddling
    assert all(addr % 8 == 4 and "v_pk_fma_f32" in line for addr, line in r["straddling"])
    assert r["tail"][-2:] == ["s_cmp_lg_u32", "s_cbranch_scc1"]
    assert loop_layout.kernel_loops(listing(sizes), "kern", depth=2)[1] == []


def test_headline_loop_has_no_straddling_instruction():
    """k_chain<float, 8, 16, reg, 13, HMC>, default build: its only depth-3 loop is hmc_interior_rs16."""
    name, reports = loop_layout.kernel_loops(loop_layout.unit_disassembly("f32", 8), loop_layout.HEADLINE, depth=3)
    assert len(reports) == 1, (name, len(reports))
    r = reports[0]
    print(name, {k: v for k, v in r.items() if k not in ("straddling", "sizes")}, len(r["straddling"]))
    assert r["contiguous"] and r["first"] % 64 == 0
    assert r["straddling"] == []
    assert r["instructions"] <= 174
    assert r["tail"][-1].startswith("s_cbranch")  # the loop's only lone 4-byte instruction is its last
    # the 4-byte vector instructions (v_exp_f32 / v_rcp_f32 of the twisted pairs) come in adjacent pairs of one kind
    sizes = r["sizes"]
    k = 0
    while k < len(sizes):
        mnem, size = sizes[k]
        if size == 4 and mnem.startswith("v_"):
            assert k + 1 < len(sizes) and sizes[k + 1] == (mnem, 4), (k, sizes[max(0, k - 2):k + 3])
            k += 2
        else:
            k += 1
    assert sum(1 for m, z in sizes if z == 4 and m.startswith("v_")) == 24
