// lr_nuts_sched.h -- the host side of NUTS on the stepwise engine as pure functions (no HIP, no device): which leaf launch comes next,
// where the host reads the tally of building chains, and how the workspace behind the stepwise engine's is carved.  lr_engine.h drives
// the launches of lr_tall_nuts.h with them; tests/host/nuts_sched_harness.cpp checks them on the CPU.
//
// Every chain of a call starts an iteration together and a building chain takes one leaf per pass; a subtree ends early only through a
// divergence or a U-turn, and both end the tree.  So every chain that is still building is at the same doubling d and leaf i of it:
// step s = 2^d - 1 + i.  The schedule is that recurrence; the device reports nothing but how many chains are still building, and the
// host asks only at the end of a doubling (s = 2^(d+1) - 2).  A count of zero ends the iteration; whatever the counts, it ends after
// 2^max_depth - 1 steps.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lr {

struct NutsStep {
    int s, d, i;  // leaf s of the iteration = leaf i of doubling d
    int last;     // the leaf ends doubling d
    int read;     // the host reads the tally after this leaf (the end of a doubling that is not the last possible one)
};

struct NutsSched {
    int max_depth, s = 0, d = 0, i = 0;
    bool stopped = false;
    explicit NutsSched(int md) : max_depth(md) {}
    bool done() const { return stopped || s >= (1 << max_depth) - 1; }
    NutsStep cur() const {
        const int last = i == (1 << d) - 1;
        return NutsStep{s, d, i, last, last && d + 1 < max_depth};
    }
    // after the launches of cur(); `building`: the tally read there (ignored where cur().read is 0)
    void advance(uint32_t building) {
        const NutsStep c = cur();
        if (c.read && building == 0) stopped = true;
        if (c.last) { ++d; i = 0; }
        else ++i;
        ++s;
    }
};

// host waits of one iteration: at most this many, whatever the device reports
inline int nuts_sched_max_reads(int max_depth) { return max_depth - 1; }

// The workspace of NUTS behind the stepwise engine's own (lr_engine.h setup_tall), every piece aligned to 256 bytes:
// vectors [kNutsTallVecs + 2 max_depth][C][P] | per-chain scalars [C][waves per chain] | tally [kNutsTallSlots]
constexpr int kNutsTallVecs = 15;    // lr_tall_nuts.h NutsTallVec
constexpr int kNutsTallSlots = 16;   // one tally per doubling (max_depth <= 10)
constexpr size_t kNutsTallChainBytes = 112;  // sizeof(NutsTallChain)
constexpr int nuts_tall_waves_per_chain(int P) { return P > 64 ? P / 64 : 1; }  // each wave of a chain keeps a record of its own (lr_tall_nuts.h)
struct NutsTallCarve { size_t vec_off, vec_bytes, chain_off, chain_bytes, tally_off, tally_bytes, total; };
inline NutsTallCarve nuts_tall_carve(int64_t C, int P, size_t esize, int max_depth) {
    auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
    NutsTallCarve c{};
    c.vec_off = 0;
    c.vec_bytes = align((size_t)(kNutsTallVecs + 2 * max_depth) * (size_t)C * (size_t)P * esize);
    c.chain_off = c.vec_off + c.vec_bytes;
    c.chain_bytes = align((size_t)C * (size_t)nuts_tall_waves_per_chain(P) * kNutsTallChainBytes);
    c.tally_off = c.chain_off + c.chain_bytes;
    c.tally_bytes = align((size_t)kNutsTallSlots * sizeof(uint32_t));
    c.total = c.tally_off + c.tally_bytes;
    return c;
}

}  // namespace lr
