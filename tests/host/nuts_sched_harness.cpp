// nuts_sched_harness.cpp -- TEST INFRASTRUCTURE: the launch schedule and the workspace carve of NUTS on the stepwise engine
// (logreg_amd/csrc/lr_nuts_sched.h) as a host program with its own main: no GPU, no HIP.  tests/test_nuts_tall_cpu.py builds it with
// -fsanitize=address,undefined and runs it.
//   - (d, i) of every step s up to 1023 equal the recurrence of nuts_run (lr_nuts.h) for a chain that keeps building: i = next ? 0 : i + 1,
//     d = next ? d + 1 : d, next at i = 2^d - 1; the checkpoint indices the kernel derives from i stay inside 2 max_depth vectors
//   - the host reads the tally only at s = 2^(d+1) - 2, never at the last possible doubling, at most max_depth - 1 times
//   - a tally that never reaches zero ends the iteration after exactly 2^max_depth - 1 steps; a zero at doubling k after 2^(k+1) - 1
//   - the carve: pieces aligned to 256 bytes, disjoint, in order, large enough for (15 + 2 max_depth) C P elements, the chain records
//     (one per wave of a chain: two at P = 128) and the tallies, for P = 4 .. 128, both element sizes and chain counts that are no multiple of anything
// Prints one line per check that failed and "nuts_sched: N checks, F failures".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lr_nuts_sched.h"

static long g_checks = 0, g_fail = 0;
#define EXPECT(c, ...) do { ++g_checks; if (!(c)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the schedule of one iteration as a list: tallies[k] is what the device reports at the end of doubling k
static std::vector<lr::NutsStep> run(int max_depth, const std::vector<uint32_t>& tallies, int* reads) {
    std::vector<lr::NutsStep> out;
    *reads = 0;
    for (lr::NutsSched sch(max_depth); !sch.done();) {
        const lr::NutsStep st = sch.cur();
        out.push_back(st);
        *reads += st.read;
        sch.advance(st.read ? tallies[(size_t)st.d] : 12345u);  // (a value where nothing is read must change nothing)
        if (out.size() > 5000) break;
    }
    return out;
}

int main() {
    for (int md = 1; md <= 10; ++md) {
        int reads = 0;
        const std::vector<uint32_t> never(16, 0xFFFFFFFFu);  // a tally that never reaches zero (a wrong count, a NaN-ridden run)
        const auto steps = run(md, never, &reads);
        EXPECT((long)steps.size() == (1L << md) - 1, "max_depth %d: %zu steps under a tally that never reaches zero", md, steps.size());
        EXPECT(reads == md - 1 && reads <= lr::nuts_sched_max_reads(md), "max_depth %d: %d reads", md, reads);
        int d = 0, i = 0;  // nuts_run's recurrence for a building chain
        for (size_t s = 0; s < steps.size(); ++s) {
            const lr::NutsStep& st = steps[s];
            EXPECT(st.s == (int)s && st.d == d && st.i == i, "max_depth %d step %zu: (s, d, i) = (%d, %d, %d), recurrence (%d, %d)", md, s, st.s, st.d, st.i, d, i);
            EXPECT(st.s == (1 << st.d) - 1 + st.i, "step %zu is not leaf i of doubling d", s);
            const bool last = i == (1 << d) - 1;
            EXPECT((st.last != 0) == last, "max_depth %d step %zu: last", md, s);
            EXPECT((st.read != 0) == (last && d + 1 < md), "max_depth %d step %zu: read", md, s);
            if (st.read) EXPECT(st.s == (1 << (st.d + 1)) - 2, "max_depth %d: a read at step %d of doubling %d", md, st.s, st.d);
            // the kernel's checkpoint indices (lr_tall_nuts.h): inside [0, max_depth) -- 2 max_depth vectors are carved
            const int idx_max = __builtin_popcount((unsigned)i >> 1), idx_min = idx_max - __builtin_ctz(~(unsigned)i) + 1;
            EXPECT(idx_max >= 0 && idx_max < md && (((i & 1) == 0) || (idx_min >= 0 && idx_min <= idx_max)), "max_depth %d leaf %d: checkpoints %d..%d", md, i, idx_min,
                   idx_max);
            const bool next = last;
            d = next ? d + 1 : d;
            i = next ? 0 : i + 1;
        }
        for (int k = 0; k + 1 < md; ++k) {  // every chain done at the end of doubling k
            std::vector<uint32_t> t(16, 7u);
            t[(size_t)k] = 0;
            const auto st = run(md, t, &reads);
            EXPECT((long)st.size() == (1L << (k + 1)) - 1 && reads == k + 1, "max_depth %d, zero at doubling %d: %zu steps, %d reads", md, k, st.size(), reads);
        }
    }
    const int Ps[] = {4, 8, 16, 32, 64, 128};
    const long long Cs[] = {1, 3, 65, 257, 1000, 4194240};
    for (int P : Ps)
        for (size_t es : {(size_t)4, (size_t)8})
            for (long long C : Cs)
                for (int md = 1; md <= 10; ++md) {
                    const lr::NutsTallCarve c = lr::nuts_tall_carve(C, P, es, md);
                    const size_t vec = (size_t)(lr::kNutsTallVecs + 2 * md) * (size_t)C * (size_t)P * es;
                    EXPECT(c.vec_off == 0 && c.vec_bytes >= vec && c.vec_bytes < vec + 256, "P %d C %lld: vectors %zu for %zu", P, C, c.vec_bytes, vec);
                    EXPECT(c.chain_off == c.vec_off + c.vec_bytes && c.chain_bytes >= (size_t)C * (size_t)(P / 64 > 1 ? P / 64 : 1) * lr::kNutsTallChainBytes && lr::nuts_tall_waves_per_chain(P) == (P / 64 > 1 ? P / 64 : 1), "P %d C %lld: chain records", P, C);
                    EXPECT(c.tally_off == c.chain_off + c.chain_bytes && c.tally_bytes >= (size_t)md * 4 && lr::kNutsTallSlots >= md, "P %d C %lld: tallies", P, C);
                    EXPECT(c.total == c.tally_off + c.tally_bytes, "P %d C %lld: total", P, C);
                    EXPECT(c.vec_off % 256 == 0 && c.chain_off % 256 == 0 && c.tally_off % 256 == 0 && c.total % 256 == 0, "P %d C %lld: alignment", P, C);
                }
    std::printf("nuts_sched: %ld checks, %ld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
