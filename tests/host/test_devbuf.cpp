// Host-only test of the owned device buffers and of the host forms' sequence
// (coconut-rust_amd/csrc/devbuf.h) that the capi_*.cpp files run over HIP.  Here the device is simulated:
// an allocation is a host block with a guard before and a canary after it, every device operation is
// appended to a log, and the k-th operation of one kind can be made to fail.  Built with
// -fsanitize=address,undefined by tests/test_sanitizers.py (LeakSanitizer on); exits non-zero on the
// first failed check.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "devbuf.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

enum Kind { ALLOC, FREE, H2D, LAUNCH, D2H, ZERO, SYNC, NKIND };

struct SimDev {
    using Stream = int;
    static constexpr size_t kGuard = 8;
    static constexpr unsigned char kCanary = 0xC5;
    struct Op {
        Kind kind;
        void* p;
        size_t n;
        bool failed;
    };
    static inline std::vector<Op> log;
    static inline std::map<void*, size_t> live;  // device pointer -> bytes
    static inline int seen[NKIND] = {};
    static inline int fail_kind = -1, fail_at = 0;  // the fail_at-th (from 1) operation of fail_kind fails
    static inline int corrupt = 0;                  // guards or canaries found overwritten, copies out of bounds

    static void reset() {
        log.clear();
        memset(seen, 0, sizeof(seen));
        fail_kind = -1;
        fail_at = 0;
    }
    static void fail(Kind k, int at) {
        reset();
        fail_kind = k;
        fail_at = at;
    }
    // logs the operation; true if it is the one to fail
    static bool step(Kind k, void* p, size_t n) {
        const bool f = k == fail_kind && ++seen[k] == fail_at;
        log.push_back({k, p, n, f});
        return f;
    }
    static int count(Kind k) {
        int c = 0;
        for (const Op& o : log) c += o.kind == k;
        return c;
    }
    // [p, p + n) lies inside one live allocation
    static bool inside(const void* p, size_t n) {
        for (auto& a : live) {
            const char* b = (const char*)a.first;
            if ((const char*)p >= b && (const char*)p + n <= b + a.second) return true;
        }
        return false;
    }
    static bool guards_ok(void* p) {
        const unsigned char* b = (const unsigned char*)p;
        const size_t n = live.at(p);
        for (size_t i = 0; i < kGuard; i++)
            if (b[-(ptrdiff_t)kGuard + (ptrdiff_t)i] != kCanary || b[n + i] != kCanary) return false;
        return true;
    }
    // --- the policy devbuf.h needs
    static void* alloc(size_t n) {
        if (step(ALLOC, nullptr, n)) return nullptr;
        unsigned char* raw = (unsigned char*)malloc(n + 2 * kGuard);
        memset(raw, kCanary, n + 2 * kGuard);
        live[raw + kGuard] = n;
        return raw + kGuard;
    }
    static void free(void* p) {
        step(FREE, p, 0);
        if (!live.count(p) || !guards_ok(p)) corrupt++;
        live.erase(p);
        ::free((unsigned char*)p - kGuard);
    }
    static int h2d(void* d, const void* h, size_t n, Stream) {
        if (step(H2D, d, n)) return -1;
        if (!inside(d, n)) return corrupt++, -1;
        memcpy(d, h, n);
        return 0;
    }
    static int d2h(void* h, const void* d, size_t n, Stream) {
        if (step(D2H, (void*)d, n)) return -1;
        if (!inside(d, n)) return corrupt++, -1;
        memcpy(h, d, n);
        return 0;
    }
    static int zero(void* d, size_t n, Stream) {
        if (step(ZERO, d, n)) return -1;
        if (!inside(d, n)) return corrupt++, -1;
        memset(d, 0, n);
        return 0;
    }
    static int sync(Stream) { return step(SYNC, nullptr, 0) ? -1 : 0; }
};

using Buf = cc::dev::BasicDevBuf<SimDev>;
using Form = cc::dev::HostForm<SimDev>;

static void test_buffer() {
    SimDev::reset();
    {
        Buf b;
        CHECK(b.ensure(100) == 0 && b.p && b.bytes == 100);
        CHECK(b.ensure(200) == 0 && b.bytes == 200);
        // growth frees the old block before it allocates the new one
        CHECK(SimDev::log.size() == 3 && SimDev::log[0].kind == ALLOC && SimDev::log[1].kind == FREE &&
              SimDev::log[2].kind == ALLOC);
        CHECK(SimDev::live.size() == 1);
        void* p = b.p;
        CHECK(b.ensure(50) == 0 && b.p == p && b.bytes == 200 && SimDev::log.size() == 3);  // smaller: a no-op
        CHECK(b.as<unsigned char>() == (unsigned char*)p);
        // a failed allocation leaves the buffer empty, and usable again
        SimDev::fail(ALLOC, 1);
        CHECK(b.ensure(400) == -1 && !b.p && b.bytes == 0 && SimDev::live.empty());
        CHECK(b.ensure(10) == 0 && b.p && b.bytes == 10);
        // a move empties its source; move assignment frees what the target held
        Buf m(std::move(b));
        CHECK(!b.p && b.bytes == 0 && m.p && m.bytes == 10 && SimDev::live.size() == 1);
        Buf t;
        CHECK(t.ensure(20) == 0 && SimDev::live.size() == 2);
        t = std::move(m);
        CHECK(!m.p && m.bytes == 0 && t.bytes == 10 && SimDev::live.size() == 1);
        CHECK(b.ensure(5) == 0 && SimDev::live.size() == 2);  // the moved-from buffer is an empty buffer
        b.release();
        CHECK(!b.p && b.bytes == 0 && SimDev::live.size() == 1);
    }
    CHECK(SimDev::live.empty());  // the destructors freed the rest
}

// a function of the host forms' shape: three local buffers, an early return when one cannot be had
static int three_buffers(size_t n) {
    Buf a, b, c;
    if (a.ensure(n) || b.ensure(2 * n) || c.ensure(3 * n)) return -1;
    return 0;
}

static void test_early_return_frees() {
    SimDev::fail(ALLOC, 2);
    CHECK(three_buffers(64) == -1);
    CHECK(SimDev::live.empty());
    CHECK(SimDev::count(ALLOC) == 2 && SimDev::count(FREE) == 1);
    SimDev::reset();
    CHECK(three_buffers(64) == 0 && SimDev::live.empty() && SimDev::count(FREE) == 3);
}

// One host form: two uploads, a "kernel" (out[i] = in[i] + key[0], then a status), one download, wipes of
// the key and of the first `wn` bytes of the input.  The kernel runs on the host when it is launched.
struct Run {
    cc_status status = CC_OK;
    unsigned char out[32] = {};
    unsigned char in_after[32] = {};
    bool guards = false;
};
static Run host_form(cc_status kernel_status, size_t wn, bool call_finish = true) {
    Run r;
    unsigned char in[32], key[4] = {7, 7, 7, 7};
    for (int i = 0; i < 32; i++) in[i] = (unsigned char)(i + 1);
    Buf d_in, d_key, d_out, d_none;
    if (d_in.ensure(32) || d_key.ensure(4) || d_out.ensure(32)) return r.status = CC_ERR_HIP, r;
    {
        Form f(0);
        f.up(d_in, in, 32);
        f.up(d_none, nullptr, 0);  // zero-length steps: skipped, their pointers never touched
        f.up_secret(d_key, key, 4);  // the upload and the wipe of the same bytes
        f.launch([&]() -> cc_status {
            if (SimDev::step(LAUNCH, d_out.p, 32)) return CC_ERR_HIP;
            for (int i = 0; i < 32; i++) d_out.as<unsigned char>()[i] = d_in.as<unsigned char>()[i] + d_key.as<unsigned char>()[0];
            return kernel_status;
        });
        f.down(r.out, d_out, 32);
        f.down(nullptr, d_none, 0);
        f.wipe(d_none, 0);
        f.wipe(d_in, wn);
        if (call_finish) r.status = f.finish();
    }  // without finish(): the destructor wipes and synchronises
    memcpy(r.in_after, d_in.p, 32);
    r.guards = SimDev::guards_ok(d_in.p) && SimDev::guards_ok(d_key.p) && SimDev::guards_ok(d_out.p);
    return r;
}

static std::vector<Kind> kinds() {
    std::vector<Kind> k;
    for (const SimDev::Op& o : SimDev::log)
        if (o.kind != ALLOC && o.kind != FREE) k.push_back(o.kind);
    return k;
}

static void test_sequence_ok() {
    SimDev::reset();
    const Run r = host_form(CC_OK, 20);
    CHECK(r.status == CC_OK);
    // uploads, launch, downloads, wipes, exactly one synchronise; the zero-length steps appear nowhere
    const std::vector<Kind> want = {H2D, H2D, LAUNCH, D2H, ZERO, ZERO, SYNC};
    CHECK(kinds() == want && SimDev::count(SYNC) == 1);
    for (const SimDev::Op& o : SimDev::log) CHECK(o.kind == ALLOC || o.kind == FREE || o.kind == SYNC || o.n > 0);
    for (int i = 0; i < 32; i++) CHECK(r.out[i] == (unsigned char)(i + 1 + 7));
    // the wipe zeroed exactly its 20 bytes: the byte after it, the guard before it and the canary stand
    for (int i = 0; i < 20; i++) CHECK(r.in_after[i] == 0);
    for (int i = 20; i < 32; i++) CHECK(r.in_after[i] == (unsigned char)(i + 1));
    CHECK(r.guards && SimDev::corrupt == 0 && SimDev::live.empty());
    // a wipe of the whole buffer stops at the canary
    SimDev::reset();
    const Run w = host_form(CC_OK, 32);
    for (int i = 0; i < 32; i++) CHECK(w.in_after[i] == 0);
    CHECK(w.status == CC_OK && w.guards && SimDev::corrupt == 0);
}

// nothing is uploaded, launched or downloaded after the failing step; both wipes and the one
// synchronise are still queued
static void check_after_failure(Kind k) {
    size_t fi = SimDev::log.size();
    for (size_t i = 0; i < SimDev::log.size(); i++)
        if (SimDev::log[i].failed) fi = i;
    CHECK(fi < SimDev::log.size() && SimDev::log[fi].kind == k);
    if (k == H2D || k == LAUNCH || k == D2H)
        for (size_t i = fi + 1; i < SimDev::log.size(); i++)
            CHECK(SimDev::log[i].kind != H2D && SimDev::log[i].kind != LAUNCH && SimDev::log[i].kind != D2H);
    CHECK(SimDev::count(ZERO) == 2 && SimDev::count(SYNC) == 1);
    CHECK(SimDev::live.empty() && SimDev::corrupt == 0);
}

static void test_sequence_failures() {
    for (int at = 1; at <= 2; at++) {  // either upload
        SimDev::fail(H2D, at);
        CHECK(host_form(CC_OK, 20).status == CC_ERR_HIP);
        check_after_failure(H2D);
        CHECK(SimDev::count(H2D) == at && SimDev::count(LAUNCH) == 0 && SimDev::count(D2H) == 0);
    }
    SimDev::fail(LAUNCH, 1);  // the launch itself
    CHECK(host_form(CC_OK, 20).status == CC_ERR_HIP);
    check_after_failure(LAUNCH);
    CHECK(SimDev::count(D2H) == 0);
    SimDev::reset();  // a launch that reports a status of its own: that status, and no download
    CHECK(host_form(CC_ERR_LEN, 20).status == CC_ERR_LEN);
    CHECK(SimDev::count(D2H) == 0 && SimDev::count(ZERO) == 2 && SimDev::count(SYNC) == 1);
    SimDev::fail(D2H, 1);
    CHECK(host_form(CC_OK, 20).status == CC_ERR_HIP);
    check_after_failure(D2H);
    for (int at = 1; at <= 2; at++) {  // a failure only in a wipe: the other wipe still runs
        SimDev::fail(ZERO, at);
        const Run r = host_form(CC_OK, 20);
        CHECK(r.status == CC_ERR_HIP);
        check_after_failure(ZERO);
        for (int i = 0; i < 32; i++) CHECK(r.out[i] == (unsigned char)(i + 1 + 7));  // the work itself was done
    }
    SimDev::fail(SYNC, 1);  // a failure only in the synchronise
    CHECK(host_form(CC_OK, 20).status == CC_ERR_HIP);
    check_after_failure(SYNC);
    // the first failing status wins: a launch status followed by a failing wipe / synchronise
    SimDev::fail(ZERO, 1);
    CHECK(host_form(CC_ERR_LEN, 20).status == CC_ERR_LEN);
    CHECK(SimDev::count(ZERO) == 2 && SimDev::count(SYNC) == 1 && SimDev::count(D2H) == 0);
    SimDev::fail(SYNC, 1);
    CHECK(host_form(CC_ERR_LEN, 20).status == CC_ERR_LEN);
}

// a form that is dropped without finish() (an early return) still wipes and synchronises
static void test_unfinished_form() {
    SimDev::reset();
    const Run r = host_form(CC_OK, 20, /*call_finish=*/false);
    CHECK(SimDev::count(ZERO) == 2 && SimDev::count(SYNC) == 1);
    for (int i = 0; i < 20; i++) CHECK(r.in_after[i] == 0);
    SimDev::reset();
    (void)host_form(CC_OK, 20);
    CHECK(SimDev::count(ZERO) == 2 && SimDev::count(SYNC) == 1);  // finish() ran once, not again on exit
}

// a device form (sync = false) leaves its work and its wipes queued; a secret download is wiped behind it
static void test_device_form_and_secret_download() {
    SimDev::reset();
    unsigned char host[8] = {}, src[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    Buf d;
    CHECK(d.ensure(8) == 0);
    {
        Form f(0, /*sync=*/false);
        f.up(d, src, 8);
        f.down_secret(host, d, 8);
        CHECK(f.finish() == CC_OK);
    }
    CHECK(kinds() == (std::vector<Kind>{H2D, D2H, ZERO}));
    CHECK(host[7] == 8 && d.as<unsigned char>()[0] == 0 && d.as<unsigned char>()[7] == 0 && SimDev::guards_ok(d.p));
    SimDev::fail(ZERO, 1);  // without a synchronise a failed wipe is still CC_ERR_HIP
    Form g(0, false);
    g.wipe(d, 8);
    CHECK(g.finish() == CC_ERR_HIP && SimDev::count(SYNC) == 0);
}

int main() {
    test_buffer();
    test_early_return_frees();
    test_sequence_ok();
    test_sequence_failures();
    test_unfinished_form();
    test_device_form_and_secret_download();
    CHECK(SimDev::live.empty() && SimDev::corrupt == 0);
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("devbuf: all checks passed\n");
    return 0;
}
