// Who owns device memory, and the one sequence every host form of the C ABI runs.
//
//   BasicDevBuf  an owned device allocation: freed by its destructor, so a local buffer is gone on every
//                return and a context's buffers go with the context; movable, not copyable.
//   HostForm     upload, launch, download, wipe, synchronise, result.  The host forms (cc_*_batch over
//                host arrays) differ in what they copy and launch; these rules are the same for all:
//                  1. a zero-length transfer or wipe is skipped and its host pointer never touched;
//                  2. after a failed step no further upload, launch or download is queued;
//                  3. every registered wipe is queued and the stream synchronised, whatever happened
//                     (a device form, which leaves its work queued, passes sync = false);
//                  4. the result is the first failing status; a wipe or synchronise failing after
//                     success is CC_ERR_HIP.
//
// No HIP types here: the device is a policy class, as in slots.h.  Dev provides Stream and the statics
//   void* alloc(size_t)   nullptr on failure          void free(void*)
//   int h2d(void* d, const void* h, size_t, Stream)   int d2h(void* h, const void* d, size_t, Stream)
//   int zero(void* d, size_t, Stream)                 int sync(Stream)               (0: ok)
// ctx.h instantiates both over hipMalloc / hipMemcpyAsync (HipMem); tests/host/test_devbuf.cpp
// over a simulated device that logs every operation and can fail the k-th one, built with
// -fsanitize=address,undefined (tests/test_sanitizers.py).
#pragma once
#include <assert.h>
#include <stddef.h>

#include "../../include/coconut_hip.h"

namespace cc {
namespace dev __attribute__((visibility("hidden"))) {

template <class Dev>
struct BasicDevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    BasicDevBuf() = default;
    BasicDevBuf(const BasicDevBuf&) = delete;
    BasicDevBuf& operator=(const BasicDevBuf&) = delete;
    BasicDevBuf(BasicDevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    BasicDevBuf& operator=(BasicDevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, bytes = o.bytes;
            o.p = nullptr, o.bytes = 0;
        }
        return *this;
    }
    ~BasicDevBuf() { release(); }
    // at least `want` bytes (contents are not kept): the old allocation is freed first, and a failed
    // allocation leaves the buffer empty
    int ensure(size_t want) {
        if (want <= bytes) return 0;
        release();
        if (!(p = Dev::alloc(want))) return -1;
        bytes = want;
        return 0;
    }
    void release() {
        if (p) Dev::free(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

template <class Dev>
class HostForm {
    using Buf = BasicDevBuf<Dev>;
    struct Wipe {
        void* p;
        size_t n;
    };
    typename Dev::Stream st_;
    cc_status s_ = CC_OK;
    bool done_ = false;
    bool sync_;
    Wipe wipes_[8];  // no form wipes more buffers
    int nwipes_ = 0;
    static cc_status status(cc_status s) { return s; }
    static cc_status status(int rc) { return rc ? CC_ERR_HIP : CC_OK; }

public:
    explicit HostForm(typename Dev::Stream st, bool sync = true) : st_(st), sync_(sync) {}
    HostForm(const HostForm&) = delete;
    HostForm& operator=(const HostForm&) = delete;
    ~HostForm() {
        if (!done_) (void)finish();  // an early return still wipes and synchronises
    }
    void up(const Buf& d, const void* h, size_t n) {
        assert(n <= d.bytes);
        if (n && !s_ && Dev::h2d(d.p, h, n, st_)) s_ = CC_ERR_HIP;
    }
    // f() queues the kernels and returns a cc_status, or a launcher's int (non-zero: CC_ERR_HIP)
    template <class F>
    void launch(F f) {
        if (!s_) s_ = status(f());
    }
    void down(void* h, const Buf& d, size_t n) {
        assert(n <= d.bytes);
        if (n && !s_ && Dev::d2h(h, d.p, n, st_)) s_ = CC_ERR_HIP;
    }
    // the first n bytes of d are zeroed behind everything queued, in finish()
    void wipe(const Buf& d, size_t n) {
        assert(n <= d.bytes && (!n || nwipes_ < 8));
        if (n) wipes_[nwipes_++] = {d.p, n};
    }
    // a secret's device copy: the transfer, and the wipe of the same bytes
    void up_secret(const Buf& d, const void* h, size_t n) { up(d, h, n), wipe(d, n); }
    void down_secret(void* h, const Buf& d, size_t n) { down(h, d, n), wipe(d, n); }
    cc_status finish() {
        done_ = true;
        bool ok = true;
        for (int i = 0; i < nwipes_; i++) ok = Dev::zero(wipes_[i].p, wipes_[i].n, st_) == 0 && ok;
        if (sync_) ok = Dev::sync(st_) == 0 && ok;
        return s_ ? s_ : ok ? CC_OK : CC_ERR_HIP;
    }
};

}  // namespace dev
}  // namespace cc
