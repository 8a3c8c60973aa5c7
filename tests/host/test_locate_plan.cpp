// Drives the locate drivers' planning function (coconut-rust_amd/csrc/locate_plan.h) on the host, built with
// -fsanitize=address,undefined by tests/test_rlc_locate_model.py.
//   test_locate_plan                    the built-in cases; prints "all checks passed"
//   test_locate_plan N SEG ACCEPTBITS   one plan for the test to compare with its own restatement: the
//                                       line "segments rejected rechecked in_place", then "lo hi off" a run
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "locate_plan.h"

using cc::locate::Plan;
using cc::locate::Run;

static int failures = 0;
#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);   \
            failures++;                                             \
        }                                                           \
    } while (0)

// accept bytes in a heap block of exactly S bytes: a read past the last segment is a sanitizer report
static Plan plan_of(size_t n, size_t seg, const std::string& bits) {
    const size_t S = cc::locate::segments(n, seg);
    if (bits.size() != S) {
        printf("FAILED: %zu accept bits for %zu segments\n", bits.size(), S);
        exit(2);
    }
    uint8_t* a = (uint8_t*)malloc(S ? S : 1);
    for (size_t s = 0; s < S; s++) a[s] = bits[s] == '1' ? 1 : 0;
    Plan p = cc::locate::plan(n, seg, a);
    free(a);
    return p;
}

// what every plan must satisfy, whatever the accept bytes
static void invariants(const Plan& p, size_t n, size_t seg, const std::string& bits) {
    size_t off = 0, prev_hi = 0, rej = 0;
    for (size_t i = 0; i < p.runs.size(); i++) {
        const Run& r = p.runs[i];
        CHECK(r.lo < r.hi && r.hi <= n);
        CHECK(r.lo % seg == 0 && (r.hi % seg == 0 || r.hi == n));
        CHECK(r.off == off);
        if (i) CHECK(r.lo > prev_hi);  // adjacent rejected segments are ONE run
        for (size_t s = r.lo / seg; s * seg < r.hi; s++) CHECK(bits[s] == '0');
        off += r.hi - r.lo;
        prev_hi = r.hi;
    }
    for (char c : bits) rej += c == '0';
    CHECK(p.rechecked == off);
    CHECK(p.rejected == rej);
    CHECK(p.segments == bits.size());
    CHECK(p.in_place() == (rej == bits.size() && rej > 0));
}

static void builtin() {
    {  // no segment rejected
        const Plan p = plan_of(150, 16, "1111111111");
        invariants(p, 150, 16, "1111111111");
        CHECK(p.segments == 10 && p.rejected == 0 && p.rechecked == 0 && p.runs.empty() && !p.in_place());
    }
    {  // every segment rejected: one run over the batch, verified in place
        const Plan p = plan_of(150, 16, "0000000000");
        invariants(p, 150, 16, "0000000000");
        CHECK(p.rejected == 10 && p.rechecked == 150 && p.in_place());
        CHECK(p.runs.size() == 1 && p.runs[0].lo == 0 && p.runs[0].hi == 150 && p.runs[0].off == 0);
    }
    {  // alternating: no two merge
        const Plan p = plan_of(128, 16, "01010101");
        invariants(p, 128, 16, "01010101");
        CHECK(p.runs.size() == 4 && p.rechecked == 64 && !p.in_place());
        for (size_t i = 0; i < 4; i++) CHECK(p.runs[i].lo == 32 * i && p.runs[i].hi == 32 * i + 16 && p.runs[i].off == 16 * i);
    }
    {  // adjacent rejected segments merge; a far one does not
        const Plan p = plan_of(150, 16, "1100111011");
        invariants(p, 150, 16, "1100111011");
        CHECK(p.runs.size() == 2 && p.rejected == 3 && p.rechecked == 48);
        CHECK(p.runs[0].lo == 32 && p.runs[0].hi == 64 && p.runs[0].off == 0);
        CHECK(p.runs[1].lo == 112 && p.runs[1].hi == 128 && p.runs[1].off == 32);
    }
    {  // the short tail segment, alone and merged with its neighbour
        Plan p = plan_of(150, 16, "1111111110");
        invariants(p, 150, 16, "1111111110");
        CHECK(p.runs.size() == 1 && p.runs[0].lo == 144 && p.runs[0].hi == 150 && p.rechecked == 6);
        p = plan_of(150, 16, "1111111100");
        invariants(p, 150, 16, "1111111100");
        CHECK(p.runs.size() == 1 && p.runs[0].lo == 128 && p.runs[0].hi == 150 && p.rechecked == 22);
    }
    {  // S = 1, accepted and rejected; a segment longer than the batch
        Plan p = plan_of(7, 16, "1");
        invariants(p, 7, 16, "1");
        CHECK(p.segments == 1 && p.runs.empty());
        p = plan_of(7, 16, "0");
        invariants(p, 7, 16, "0");
        CHECK(p.in_place() && p.rechecked == 7 && p.runs.size() == 1 && p.runs[0].hi == 7);
    }
    {  // an empty batch reads no accept byte
        const Plan p = cc::locate::plan(0, 16, nullptr);
        CHECK(p.segments == 0 && p.runs.empty() && !p.in_place());
    }
    // the segment lengths the segmented partial takes
    CHECK(!cc::locate::valid_seg(0, 1 << 26) && !cc::locate::valid_seg(2, 1 << 26) && !cc::locate::valid_seg(3, 1 << 26));
    CHECK(!cc::locate::valid_seg(6, 1 << 26) && !cc::locate::valid_seg((size_t)1 << 27, 1 << 26));
    CHECK(cc::locate::valid_seg(4, 1 << 26) && cc::locate::valid_seg(4096, 1 << 26) && cc::locate::valid_seg(1 << 26, 1 << 26));
    CHECK(cc::locate::log2_exact(4) == 2 && cc::locate::log2_exact(4096) == 12);
    CHECK(cc::locate::valid_seg(cc::locate::default_seg(0), 1 << 26) && cc::locate::valid_seg(cc::locate::default_seg(1), 1 << 26));
    CHECK(cc::locate::segments(150, 16) == 10 && cc::locate::segments(64, 16) == 4 && cc::locate::segments(1, 4) == 1);
}

int main(int argc, char** argv) {
    if (argc == 4) {
        const size_t n = strtoull(argv[1], nullptr, 10), seg = strtoull(argv[2], nullptr, 10);
        const std::string bits = argv[3];
        const Plan p = plan_of(n, seg, bits);
        invariants(p, n, seg, bits);
        printf("%zu %zu %zu %d\n", p.segments, p.rejected, p.rechecked, p.in_place() ? 1 : 0);
        for (const Run& r : p.runs) printf("%zu %zu %zu\n", r.lo, r.hi, r.off);
        return failures ? 1 : 0;
    }
    builtin();
    if (failures) return 1;
    printf("all checks passed\n");
    return 0;
}
