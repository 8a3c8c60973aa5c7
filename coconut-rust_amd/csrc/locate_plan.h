// Host-only planning of the RLC locate drivers (cc_verify_batch_locate*, capi_locate.cpp): the batch of n
// credentials is checked in S = ceil(n / seg) segments, each with its own accept byte; the rejected
// segments are verified per credential in ONE launch sequence over a compacted copy of their rows.  From
// the accept bytes, plan() gives the merged runs [lo, hi) of rejected credentials (adjacent rejected
// segments are one run: one device-to-device copy per array instead of one per segment), each run's
// offset in the compacted workspace, and the counts the drivers report.
//
// No HIP types here, as in slots.h: tests/host/test_locate_plan.cpp drives it under
// -fsanitize=address,undefined (tests/test_rlc_locate_model.py, `pytest -m "not gpu"`).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace cc {
namespace locate {

// the library's segment length for seg = 0, per group mode (coconut_hip.h CC_LOCATE_SEG_DEFAULT_G2 / _G1;
// the measurement behind them: DESIGN.md, "RLC locate")
constexpr size_t kDefaultSegG2 = 4096, kDefaultSegG1 = 1024;
inline size_t default_seg(int mode) { return mode == 0 ? kDefaultSegG2 : kDefaultSegG1; }

// a segment length the segmented partial takes: a power of two in [4, max_seg] (four credentials share a
// Miller value, and the product tree passes through the level of seg / 4 values only for powers of two)
inline bool valid_seg(size_t seg, size_t max_seg) { return seg >= 4 && seg <= max_seg && (seg & (seg - 1)) == 0; }
inline size_t segments(size_t n, size_t seg) { return (n + seg - 1) / seg; }
inline int log2_exact(size_t seg) {
    int k = 0;
    while (((size_t)1 << k) < seg) k++;
    return k;
}

struct Run {
    size_t lo, hi;  // credentials [lo, hi) of the batch
    size_t off;     // their first row in the compacted workspace
};
struct Plan {
    size_t segments = 0;   // S
    size_t rejected = 0;   // segments whose accept byte is clear
    size_t rechecked = 0;  // credentials in them (= the compacted rows)
    std::vector<Run> runs;
    // every segment rejected: the whole batch is verified where it lies, nothing is compacted
    bool in_place() const { return segments && rejected == segments; }
};

// accept: S bytes, non-zero = the segment's RLC check passed
inline Plan plan(size_t n, size_t seg, const uint8_t* accept) {
    Plan p;
    if (!n || !seg) return p;
    p.segments = segments(n, seg);
    for (size_t s = 0; s < p.segments; s++) {
        if (accept[s]) continue;
        const size_t lo = s * seg, hi = lo + seg < n ? lo + seg : n;
        p.rejected++;
        if (!p.runs.empty() && p.runs.back().hi == lo) p.runs.back().hi = hi;
        else p.runs.push_back(Run{lo, hi, p.rechecked});
        p.rechecked += hi - lo;
    }
    return p;
}

}  // namespace locate
}  // namespace cc
