// Host-only test of the concurrency-slot bookkeeping (coconut-rust_amd/csrc/slots.h) that the capi_*.cpp
// files run over HIP (csrc/ctx.h HipDev).  Here the device is simulated: every stream is a FIFO of queued
// operations, an event marks a stream position, a "kernel" reads a set of buffers (id + allocation
// generation), and a buffer reallocated while a queued operation still reads its old allocation is counted
// as a use-after-free (what the GPU would do with a hipFree'd workspace).  A queued copy of the pinned
// upload ring (Staging) reads its source only when its stream runs, and the pinned blocks are heap blocks:
// an entry reused too early shows as wrong bytes, a block freed too early as an AddressSanitizer report.
// Built with -fsanitize=address,undefined by tests/test_sanitizers.py; exits non-zero on a failed check.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <map>
#include <vector>

#include "slots.h"

using namespace cc::slots;

static int g_fail = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

struct FakeBuf {
    int id = 0;
    size_t bytes = 0;
    int gen = 0;
};

struct FakeDev {
    using Buf = FakeBuf;
    using Event = int;   // index into evs (0: not created)
    using Stream = int;  // index into streams
    struct Op {
        long seq;
        std::vector<std::pair<int, int>> reads;  // (buffer id, generation)
        int wait_stream = -1;                    // a wait: completes after that stream reaches wait_seq
        long wait_seq = -1;
        void* dst = nullptr;  // a copy: n bytes of src to dst when the operation runs
        const void* src = nullptr;
        size_t n = 0;
    };
    std::vector<std::deque<Op>> streams;
    std::map<int, std::pair<int, long>> evs;  // event -> (stream, seq of its last op when recorded)
    long seq = 0;
    int next_buf = 1, next_ev = 1;
    int uaf = 0;       // reallocations under a queued reader
    int bad_read = 0;  // kernels launched on a null / undersized workspace

    explicit FakeDev(int nstreams) : streams((size_t)nstreams) {}
    Event new_event() { return next_ev++; }
    void name(FakeBuf& b) {
        if (!b.id) b.id = next_buf++;
    }
    bool read_pending(int id, int gen) const {
        for (const auto& q : streams)
            for (const Op& o : q)
                for (auto& r : o.reads)
                    if (r.first == id && r.second == gen) return true;
        return false;
    }
    // --- the policy slots.h needs
    int ensure(FakeBuf& b, size_t n) {
        name(b);
        if (n <= b.bytes) return 0;
        if (b.bytes && read_pending(b.id, b.gen)) uaf++;
        b.gen++;
        b.bytes = n;
        return 0;
    }
    int record(Event e, Stream s) {
        if (hit()) return failed_record = true, -1;
        if (!e) return -1;
        evs[e] = {s, streams[(size_t)s].empty() ? -1 : streams[(size_t)s].back().seq};
        return 0;
    }
    int wait(Stream s, Event e) {
        auto it = evs.find(e);
        if (it == evs.end()) return 0;  // never recorded: nothing to wait for
        Op o;
        o.seq = ++seq;
        o.wait_stream = it->second.first;
        o.wait_seq = it->second.second;
        streams[(size_t)s].push_back(o);
        return 0;
    }
    int sync(Event e) {
        if (hit()) return -1;
        auto it = evs.find(e);
        if (it == evs.end()) return 0;
        run_until(it->second.first, it->second.second);
        return 0;
    }
    // --- and Staging: the calls are counted and the fail_at-th fails (Pool's tests never set it)
    int calls = 0, fail_at = -1, live_events = 0, live_pins = 0;
    bool failed_record = false;
    bool hit() { return calls++ == fail_at; }
    void* pin(size_t n) {
        if (hit()) return nullptr;
        live_pins++;
        return malloc(n);
    }
    void unpin(void* p) {
        live_pins--;
        free(p);
    }
    int create(Event& e) {
        if (hit()) return -1;
        live_events++;
        e = new_event();
        return 0;
    }
    void destroy(Event) { live_events--; }
    int h2d(void* d, const void* h, size_t n, Stream s) {
        if (hit()) return -1;
        Op o;
        o.seq = ++seq;
        o.dst = d, o.src = h, o.n = n;
        streams[(size_t)s].push_back(o);
        return 0;
    }
    // --- the simulated device
    // completes stream s's operations up to seq (waits first complete what they wait for)
    void run_until(int s, long upto) {
        auto& q = streams[(size_t)s];
        while (!q.empty() && q.front().seq <= upto) {
            Op o = q.front();
            if (o.wait_stream >= 0) run_until(o.wait_stream, o.wait_seq);
            if (o.n) memcpy(o.dst, o.src, o.n);
            q.pop_front();
        }
    }
    void run_all() {
        for (size_t s = 0; s < streams.size(); s++) run_until((int)s, seq);
    }
    // a kernel on stream s reading the workspaces w needs for sizes sz
    void launch(Stream s, const Work<FakeBuf>& w, const Sizes& sz) {
        Op o;
        o.seq = ++seq;
        for (int k = 0; k < Work<FakeBuf>::kN; k++) {
            FakeBuf* b = w.at(k);
            if (!b || b->bytes < sz.at(k)) {
                bad_read++;
                continue;
            }
            if (sz.at(k)) o.reads.push_back({b->id, b->gen});
        }
        streams[(size_t)s].push_back(o);
    }
};

// a context's slot 0 (its own workspaces) + K-1 slot buffer sets, as capi_ctx.cpp cc_set_concurrency builds
struct Ctx {
    FakeDev dev;
    Pool<FakeDev> pool;
    SlotBufs<FakeBuf> own;
    std::vector<SlotBufs<FakeBuf>*> extra;
    FakeDev::Event order_ev;
    static constexpr int kCtxStream = 0;
    Ctx(int K, int nstreams) : dev(nstreams) {
        order_ev = dev.new_event();
        pool.recs.resize((size_t)K);
        pool.recs[0].w = own.work();
        pool.recs[0].done = dev.new_event();
        for (int k = 1; k < K; k++) {
            extra.push_back(new SlotBufs<FakeBuf>);
            pool.recs[(size_t)k].w = extra.back()->work();
            pool.recs[(size_t)k].done = dev.new_event();
        }
    }
    ~Ctx() {
        for (auto* e : extra) delete e;
    }
    // one verify batch as capi_verify.cpp verify_device runs it on a slot; fail_after: the launch "fails" after
    // queueing that many kernels (the Fence must still end the slot)
    int batch(int stream, size_t n, size_t vkw = 0, int fail_after = -1, bool use_fence = true) {
        const Sizes sz = verify_sizes(n, vkw, 0, 0);
        const int k = pool.take();
        const int rc = pool.begin(dev, k, sz, stream, kCtxStream, order_ev);
        if (rc) return rc;
        if (!use_fence) {  // the pre-Fence code path: a failed launch returned without recording done
            for (int j = 0; j < 3; j++) {
                if (j == fail_after) return -7;
                dev.launch(stream, pool.recs[(size_t)k].w, sz);
            }
            return pool.end(dev, k, stream);
        }
        Fence<FakeDev> fence(pool, dev, k, stream);
        for (int j = 0; j < 3; j++) {  // prep, Miller, fexp
            if (j == fail_after) return -7;
            dev.launch(stream, pool.recs[(size_t)k].w, sz);
        }
        return fence.close();
    }
};

static void test_sizes() {
    const Sizes a = verify_sizes(100, 0, 0, 0);
    CHECK(a.prep == 100 * 12 * 4 * kPrepSlots && a.flags == 400 && a.fbuf == 100 * 12 * 4 * 12);
    CHECK(a.scratch == 72 * 12 * 100 * 4);  // k_fexp1's chain below kFexpWideMax
    CHECK(a.wprep == 200 * 12 * 4 * kPrepSlots && a.wflags == 800 && a.wf == 200 * 12 * 4 * 12);
    const Sizes b = verify_sizes(kWideMax + 1, 123, 0, 8);
    CHECK(b.scratch == 0 && b.wprep == 0 && b.wflags == 0 && b.wf == 0 && b.vkb == 123 && b.idx == 8);
    const Sizes c = verify_sizes(kFexpWideMax + 1, 0, 0, 0);
    CHECK(c.scratch == 0 && c.wprep > 0);  // the wide Miller path reaches further than the wide fexp
}

static void test_work_complete() {
    SlotBufs<FakeBuf> s;
    Work<FakeBuf> w = s.work();
    CHECK(w.complete());
    for (int k = 0; k < Work<FakeBuf>::kN; k++) {
        Work<FakeBuf> v = w;
        // knock out workspace k (what round 5's partial aggregate did for scratch / idx)
        FakeBuf** m[] = {&v.prep, &v.flags, &v.fbuf, &v.vkb, &v.scratch, &v.idx, &v.wprep, &v.wflags, &v.wf};
        *m[k] = nullptr;
        CHECK(!v.complete());
        // a pool slot holding it refuses the batch instead of launching on a null workspace
        FakeDev dev(2);
        Pool<FakeDev> p;
        p.recs.resize(1);
        p.recs[0].w = v;
        p.recs[0].done = dev.new_event();
        CHECK(p.begin(dev, 0, verify_sizes(16, 0, 0, 0), 1, 0, dev.new_event()) == -2);
        CHECK(dev.bad_read == 0);
    }
    Work<FakeBuf> d;  // default-constructed: nothing named
    CHECK(!d.complete());
}

static void test_round_robin() {
    Ctx c(3, 4);
    int seen[3] = {0, 0, 0};
    for (int j = 0; j < 9; j++) seen[c.pool.take()]++;
    CHECK(seen[0] == 3 && seen[1] == 3 && seen[2] == 3);
}

// K = 2, batches alternating on two streams; the third batch lands on slot 0 again and is larger: the
// pool must wait for slot 0's first batch before it grows the buffers that batch still reads
static void test_reuse_waits_for_inflight() {
    Ctx c(2, 3);
    CHECK(c.batch(1, 1000) == 0);  // slot 0
    CHECK(c.batch(2, 1000) == 0);  // slot 1
    CHECK(c.dev.uaf == 0);
    CHECK(c.batch(1, 5000) == 0);  // slot 0, grows: waits for batch 1 first
    CHECK(c.batch(2, 8000, 4096) == 0);  // slot 1, grows (and a per-verkey scratch)
    CHECK(c.dev.uaf == 0 && c.dev.bad_read == 0);
    // same-size reuse: no growth, the stream waits on the device instead (no host wait, no realloc)
    const int gen0 = c.own.prep.gen;
    CHECK(c.batch(1, 5000) == 0);
    CHECK(c.own.prep.gen == gen0 && c.dev.uaf == 0);
    c.dev.run_all();
}

// the simulated device does flag the bug class: growing a slot's buffer with its batch still queued
static void test_detector_has_teeth() {
    Ctx c(2, 3);
    CHECK(c.batch(1, 1000) == 0);
    c.dev.ensure(c.own.prep, 1u << 30);  // reallocation without waiting for the slot's batch
    CHECK(c.dev.uaf == 1);
}

// a launch failing half-way: the Fence still records the slot's done behind the kernels it queued, so
// the next (larger) batch on that slot waits for them
static void test_fence_on_failure() {
    Ctx c(2, 3);
    CHECK(c.batch(1, 1000, 0, /*fail_after=*/2) == -7);
    CHECK(c.batch(2, 1000) == 0);
    CHECK(c.batch(1, 9000) == 0);
    CHECK(c.dev.uaf == 0);
    // without the fence (the pre-round-6 path) the same sequence reallocates under a queued kernel
    Ctx d(2, 3);
    CHECK(d.batch(1, 1000) == 0);
    CHECK(d.batch(2, 1000) == 0);
    CHECK(d.batch(1, 1000, 0, 2, /*use_fence=*/false) == -7);  // slot 0: kernels queued, done not recorded
    CHECK(d.batch(2, 1000) == 0);
    CHECK(d.batch(1, 9000) == 0);  // slot 0 grows, but its done marks the batch before the failed one
    CHECK(d.dev.uaf > 0);
}

// drain waits for every slot; wait_all orders a stream after every slot's last batch
static void test_drain() {
    Ctx c(3, 4);
    CHECK(c.batch(1, 500) == 0);
    CHECK(c.batch(2, 500) == 0);
    CHECK(c.batch(3, 500) == 0);
    c.pool.drain(c.dev);
    for (auto& q : c.dev.streams) CHECK(q.empty());
    // shared buffers (tables) may now be rebuilt: nothing queued reads anything
    CHECK(!c.dev.read_pending(c.own.prep.id, c.own.prep.gen));
}

// ---------------------------------------------------------------- the pinned upload ring (Staging)
// a device whose event synchronise does nothing: what the ring would be without its waits
struct NoSyncDev : FakeDev {
    using FakeDev::FakeDev;
    int sync(Event) { return 0; }
};

// one ring on stream 1 of a two-stream device, which runs only when the ring (or the test) makes it
template <class Dev>
struct Ring {
    static constexpr int kR = Staging<Dev>::kR;
    Dev dev{2};
    Staging<Dev> g;
    std::deque<std::vector<unsigned char>> want, dst;
    std::vector<bool> ok;
    // the next upload, of distinct contents; the caller's array is scribbled over as soon as the call returns
    int up(size_t len) {
        const int i = (int)want.size();
        want.emplace_back(len);
        for (size_t j = 0; j < len; j++) want.back()[j] = (unsigned char)(37 * i + (int)j + 1);
        dst.emplace_back(len, (unsigned char)0);
        std::vector<unsigned char> tmp = want.back();
        const int rc = g.upload(dev, len ? dst.back().data() : nullptr, len ? tmp.data() : nullptr, len, 1);
        std::fill(tmp.begin(), tmp.end(), (unsigned char)0xEE);
        ok.push_back(rc == 0);
        return rc;
    }
    // destinations of successful uploads that do not hold their own bytes
    int wrong() const {
        int w = 0;
        for (size_t i = 0; i < want.size(); i++) w += ok[i] && dst[i] != want[i];
        return w;
    }
    bool pending() const { return !dev.streams[1].empty(); }
    bool all_released() const { return !g.host && !g.bytes && !dev.live_pins && !dev.live_events; }
};

// case 1: kR + 3 uploads on a stream that runs only at the end; returns the wrong destinations
template <class Dev>
static int ring_reuse_wrong() {
    Ring<Dev> r;
    for (int i = 0; i < Ring<Dev>::kR + 3; i++) CHECK(r.up(24) == 0);
    CHECK(r.g.bytes == 64);  // rounded up to 64 bytes an entry
    CHECK(r.pending());      // the last kR copies are still queued
    r.dev.run_all();
    const int w = r.wrong();
    r.g.release(r.dev);
    CHECK(r.all_released());
    return w;
}

static void test_ring_reuse_waits_for_its_entry() {
    CHECK(ring_reuse_wrong<FakeDev>() == 0);
    // teeth: without the wait an entry is overwritten while its copy is queued
    CHECK(ring_reuse_wrong<NoSyncDev>() > 0);
}

// case 2: a larger upload arrives while earlier copies are queued: they run before their block is freed
static void test_ring_growth_waits_for_every_entry() {
    Ring<FakeDev> r;
    for (int i = 0; i < 3; i++) CHECK(r.up(16) == 0);
    CHECK(r.pending() && r.g.bytes == 64);
    CHECK(r.up(200) == 0);
    CHECK(r.g.bytes == 256 && r.dev.live_pins == 1);
    for (int i = 0; i < 3; i++) CHECK(r.dst[(size_t)i] == r.want[(size_t)i]);  // ran before the free
    CHECK(r.pending());  // the large one is queued
    for (int i = 0; i < Ring<FakeDev>::kR + 1; i++) CHECK(r.up(i % 2 ? 200 : 16) == 0);
    r.dev.run_all();
    CHECK(r.wrong() == 0);
    r.g.release(r.dev);
    CHECK(r.all_released());
}

// case 3: a zero-length upload makes no device call, takes no entry and touches neither pointer
static void test_ring_zero_length() {
    Ring<FakeDev> r;
    CHECK(r.up(0) == 0 && r.dev.calls == 0 && !r.g.host);
    CHECK(r.up(16) == 0);
    const int calls = r.dev.calls, next = r.g.next;
    CHECK(r.up(0) == 0 && r.dev.calls == calls && r.g.next == next);
    CHECK(r.up(16) == 0);
    r.dev.run_all();
    CHECK(r.wrong() == 0);
    r.g.release(r.dev);
    CHECK(r.all_released());
}

// case 4: every device call of a run with reuse and growth fails in turn: that upload reports it, the next
// upload and release are clean.  (A failed record leaves its copy queued with no event to wait for; the
// caller's stream is past use then, and the test lets it run before it goes on.)
static void test_ring_failures() {
    const size_t lens[] = {16, 16, 16, 16, 16, 16, 200, 16};
    int ncalls = 0;
    for (int k = -1; k < ncalls || k < 0; k++) {
        Ring<FakeDev> r;
        r.dev.fail_at = k;
        int failed = 0;
        for (size_t len : lens)
            if (r.up(len)) {
                failed++;
                break;
            }
        if (k < 0) {
            ncalls = r.dev.calls;
            CHECK(failed == 0 && ncalls > 20);
        } else {
            CHECK(failed == 1);
        }
        r.dev.fail_at = -1;
        if (r.dev.failed_record) r.dev.run_all();
        CHECK(r.up(48) == 0);
        r.dev.run_all();
        CHECK(r.wrong() == 0 && r.dst.back() == r.want.back());
        r.g.release(r.dev);
        CHECK(r.all_released());
    }
}

// case 5: release with copies queued waits for them before the block goes; the ring is usable again
static void test_ring_release_pending() {
    Ring<FakeDev> r;
    for (int i = 0; i < 3; i++) CHECK(r.up(32) == 0);
    CHECK(r.pending());
    r.g.release(r.dev);
    CHECK(r.all_released() && r.wrong() == 0);
    CHECK(r.up(32) == 0);
    r.dev.run_all();
    CHECK(r.wrong() == 0);
    r.g.release(r.dev);
    CHECK(r.all_released());
}

int main() {
    test_ring_reuse_waits_for_its_entry();
    test_ring_growth_waits_for_every_entry();
    test_ring_zero_length();
    test_ring_failures();
    test_ring_release_pending();
    test_sizes();
    test_work_complete();
    test_round_robin();
    test_reuse_waits_for_inflight();
    test_detector_has_teeth();
    test_fence_on_failure();
    test_drain();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("slots: all checks passed\n");
    return 0;
}
