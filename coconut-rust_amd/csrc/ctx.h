// Internal header of the C ABI's host side (include/coconut_hip.h), which lives in the capi_*.cpp files, one
// per area: capi_ctx (contexts, tables, timing, concurrency), capi_verify (Signature::verify, the RLC,
// device sets), capi_locate and capi_pok_locate (the RLC locate modes), capi_pok, capi_aggregate, capi_issuer, capi_holder, capi_keygen, capi_vss.  Here: the HIP policies of
// devbuf.h and slots.h, struct cc_ctx, the stream-ordering helpers, and the helpers more than one area
// calls.  The cc_* definitions take their C linkage from coconut_hip.h's declarations.  Every compute step
// runs in the HIP kernels behind launch.h — there is no CPU fallback in this library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <rccl/rccl.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/coconut_hip.h"
#include "devbuf.h"
#include "launch.h"
#include "locate_plan.h"
#include "rlc_part.h"
#include "slots.h"

namespace cc {
namespace host __attribute__((visibility("hidden"))) {

// fixed-base window tables (fixed.h): per base ceil(256 / wbits) windows of 2^wbits - 1 affine entries
static inline size_t tab_words(int group, int wbits) {
    return (size_t)((256 + wbits - 1) / wbits) * (((size_t)1 << wbits) - 1) * (group == 1 ? 24 : 48);
}
static inline size_t tab_nwin(int wbits) { return (size_t)((256 + wbits - 1) / wbits); }
// free HBM of the current device (0 if the runtime cannot say)
size_t free_hbm();
// The window width of the issuer, request and keygen tables (bytes(w) bytes at w bits): the forced width, else the
// widest of 16 / 13 / 12 / 10 bits that fits cap and half the free HBM, else 8.  Called with the old tables released,
// so their memory counts as free and identical calls pick the same width.
template <class Bytes>
static int pick_table_bits(int forced, double cap, Bytes bytes) {
    if (forced) return forced;
    const double budget = std::min(cap, 0.5 * (double)free_hbm());
    for (int cand : {16, 13, 12, 10})
        if ((double)bytes(cand) <= budget) return cand;
    return 8;
}
// ... and the allocation of theirs and of the verkey's (alloc(w): true when done).  A width whose tables exceed 0.9
// of the free HBM is refused up front: hipMalloc does not reliably fail for sizes above it (the runtime may over-
// commit), and a build kernel writing such a table would not end well.  A refused or failed width falls back to 8
// bits unless it was forced or was 8 already.  Returns the width allocated, 0 on failure.
template <class Bytes, class Alloc>
static int alloc_tables(int wb, bool forced, Bytes bytes, Alloc alloc) {
    const double fr = (double)free_hbm();
    if (!(fr > 0 && (double)bytes(wb) > 0.9 * fr) && alloc(wb)) return wb;
    (void)hipGetLastError();  // clear a failed allocation's error
    return forced || wb == 8 || !alloc(8) ? 0 : 8;
}
constexpr size_t PREP_SLOTS = cc::slots::kPrepSlots;  // soa.h

// The device policy of the owned buffers and of the host forms' sequence (devbuf.h)
struct HipMem {
    using Stream = hipStream_t;
    static void* alloc(size_t n) {
        void* p = nullptr;
        return hipMalloc(&p, n) == hipSuccess ? p : nullptr;
    }
    static void free(void* p) { (void)hipFree(p); }
    static int h2d(void* d, const void* h, size_t n, hipStream_t st) {
        return hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st) == hipSuccess ? 0 : -1;
    }
    static int d2h(void* h, const void* d, size_t n, hipStream_t st) {
        return hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, st) == hipSuccess ? 0 : -1;
    }
    static int zero(void* d, size_t n, hipStream_t st) { return hipMemsetAsync(d, 0, n, st) == hipSuccess ? 0 : -1; }
    static int sync(hipStream_t st) { return hipStreamSynchronize(st) == hipSuccess ? 0 : -1; }
};
using DevBuf = cc::dev::BasicDevBuf<HipMem>;
using HostForm = cc::dev::HostForm<HipMem>;

// The device policy of the slot bookkeeping and of a slot's pinned upload ring (slots.h): hipMalloc'd
// buffers, HIP events and streams, hipHostMalloc'd staging.
struct HipDev {
    using Buf = DevBuf;
    using Event = hipEvent_t;
    using Stream = hipStream_t;
    int ensure(DevBuf& b, size_t n) { return b.ensure(n); }
    int sync(hipEvent_t e) { return hipEventSynchronize(e) == hipSuccess ? 0 : -1; }
    int record(hipEvent_t e, hipStream_t s) { return hipEventRecord(e, s) == hipSuccess ? 0 : -1; }
    int wait(hipStream_t s, hipEvent_t e) { return hipStreamWaitEvent(s, e, 0) == hipSuccess ? 0 : -1; }
    int create(hipEvent_t& e) { return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? 0 : -1; }
    void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
    void* pin(size_t n) {
        void* p = nullptr;
        return hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    void unpin(void* p) { (void)hipHostFree(p); }
    int h2d(void* d, const void* h, size_t n, hipStream_t s) { return HipMem::h2d(d, h, n, s); }
};
using VerifyWork = cc::slots::Work<DevBuf>;
using VerifySlot = cc::slots::SlotBufs<DevBuf>;  // slots 1 .. K-1 (slot 0: the context's workspaces)
using SlotPool = cc::slots::Pool<HipDev>;
using SlotFence = cc::slots::Fence<HipDev>;
using Staging = cc::slots::Staging<HipDev>;

}  // namespace host
}  // namespace cc
using namespace cc::host;

struct cc_ctx {
    int device = 0;
    int mode = 0;  // 0 SigG2, 1 SigG1
    hipStream_t stream = nullptr;
    // params
    bool have_params = false;
    std::vector<uint8_t> gtilde_bytes;  // encoding as given (subgroup status at cc_set_verkey; idempotence)
    DevBuf gtilde_aff;   // OtherGroup affine (Montgomery, AoS)
    uint32_t gtilde_inf = 0;
    DevBuf gtilde_lines; // SigG1: Miller lines of g~
    DevBuf gtilde_lz;    // SigG2: g~ affine in the lazy field's R' form (the Miller loop's constant P)
    // verkey
    bool have_vk = false;
    size_t q = 0;
    DevBuf vk_aff;       // (q + 3) points: X~, Y~[q], g~, X~ (AoS)
    DevBuf vk_inf;       // (q + 3) flags
    DevBuf table;        // fixed-base tables for Y~[0..q), g~ and X~ (q + 2 bases; X~ for RLC)
    DevBuf table_inf;    // q + 2 base flags
    int wbits = 16;      // window width of `table`
    int force_vk_bits = 0, force_iss_bits = 0;  // cc_set_table_bits (0: chosen by memory)
    bool vk_subgroup = false;  // X~, Y~ and g~ all in the order-r subgroup (RLC soundness needs it)
    std::vector<uint8_t> vk_bytes;  // X~ || Y~ encodings of the current verkey (cc_set_verkey idempotence)
    int vk_built_force = 0;         // force_vk_bits when the current tables were built
    uint32_t X_inf = 0;
    // workspaces
    DevBuf in_s1, in_s2, in_msgs, in_vkX, in_vkY, in_aux[6];
    DevBuf prep, flags, fbuf, scratch, verdicts, gt, vkb, lag;  // vkb: per-credential-verkey MSM scratch
    DevBuf wide_prep, wide_flags, wide_f;  // batches of <= kWideMax: the one-wave-per-pair Miller path
    // RLC batch mode: ChaCha20 key, identity flag word, partial / gathered partials, verdict
    DevBuf rlc_key, rlc_any, rlc_part, rlc_flag, rlc_accept;
    // cc_rlc_finish_device's own buffers: Fp12 values (partial products, window pairs' Miller values),
    // the product tree's other half / the one-element fexp's scratch, the window pairs' prep and skip
    // flags, the combined product
    DevBuf fin_f, fin_scratch, fin_prep, fin_flags2, fin_part;
    hipEvent_t ev_fin = nullptr;  // end of the last finish: finishes of one context run in call order
    bool fin_recorded = false;
    // the segmented partial, the per-partial finish and the locate drivers (capi_locate.cpp): one fall-back
    // word per segment, the segmented fold's workspace, the per-partial flags of a finish; the drivers'
    // segment partials and accept bytes, and the compacted rows and verdicts of the rejected segments
    DevBuf seg_any, seg_work, fin_each_flags, loc_parts, loc_accept, loc_s1, loc_s2, loc_msgs, loc_verdicts;
    DevBuf loc_pok[5];  // the PoK locate driver's compacted J, T, responses, challenges, revealed messages
    // RLC g~-side fold (fold.hip): fold points, delta digits, sort/partials/bucket workspace; the fixed
    // points P_w = (256^w) g~ of the window pairs (SoA, built with the verkey tables) and their
    // identity flags
    DevBuf rlc_pts, rlc_dig, rlc_work, rlc_pw, rlc_finf;
    DevBuf pok_idx;  // revealed indices of the last PoK batch
    DevBuf prove_idx, prove_scratch;  // holder side (pok_prove.hip): revealed indices, sigma' entry tables
    // request params (cc_set_request_params): SignatureGroup fixed-base tables of [h_0 .. h_{q-1}, g] for
    // SignatureRequest::new / SignatureRequestPoK::init (sigreq_prove.hip), apart from the verkey's
    bool have_rq = false;
    size_t rq_q = 0;
    int rq_wbits = 8;
    DevBuf rq_aff, rq_inf, rq_table;
    // their workspaces: per-request (pk, h) window tables, the two-base tasks' digits, compute_h's input
    // rows, offsets and failure flag
    DevBuf rq_tab, rq_dig, rq_hdata, rq_hoff, rq_fail;
    // issuer side, device forms (issue_dev.hip): h where the caller takes none, the per-request tables of the
    // variable bases, challenge and response digits, check flags; blind signing's Straus bases, scalars,
    // interleaved outputs and the device copy of x | y
    DevBuf iv_h, iv_tab, iv_cdig, iv_dig, iv_ok, bs_pts, bs_sc, bs_out, bs_xy;
    // keygen params (cc_set_keygen_params): the OtherGroup fixed-base table of g~ and, with the Pedersen
    // generators bound, the two-base G1 table [g, h] (keygen.hip), apart from every other table; kg_io:
    // the host forms' device copies (coeffs, coeffs_t, x, y, xt, yt, comm, X, Y, and combine's inputs)
    bool have_kg = false, kg_have_gh = false;
    int kg_wbits = 8;
    DevBuf kg_gt_aff, kg_gt_inf, kg_gt_table, kg_gh_aff, kg_gh_inf, kg_gh_table, kg_io[14];
    // verify_share over commitment sets (capi_vss.cpp, vss.hip): g | h as given (the irregular sets' exact route
    // and the G1 test read the encodings), and the drivers' workspaces and plan (VssBuf)
    DevBuf kg_gh_enc, vss[20];
    std::vector<uint64_t> vss_plan;
    int n_simd = 0;  // SIMDs of the device (4 a CU), read once (pok_rlc_twin)
    // issuer table (cc_set_issuers): sorted ids, decoded verkeys, per-base 8-bit window tables
    size_t iss_n = 0, iss_q = 0;
    std::vector<uint64_t> iss_ids_host;
    DevBuf iss_ids, iss_aff, iss_inf, iss_table;
    int iss_wbits = 8;  // window width of the issuer tables
    DevBuf agg_scratch;
    DevBuf dev_err;  // device-side argument errors of *_device calls (cc_device_error)
    uint32_t rlc_key_host[8] = {0};
    // timing
    bool timing = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_ms[3] = {0, 0, 0};
    // orders a caller-supplied stream against the context stream (StreamOrder below)
    hipEvent_t ev_order = nullptr;
    // side stream (high priority; ev_fork / ev_join): Verkey::aggregate beside Signature::aggregate,
    // the RLC fold's window pairs beside the delta MSM
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // device set (cc_ctx_create_multi): one single-device context per GPU and one RCCL communicator
    // per GPU (ncclCommInitAll, this process drives every device); empty for a single-device context
    std::vector<cc_ctx*> peers;
    std::vector<ncclComm_t> comms;
    DevBuf rlc_gath;  // per peer: gathered partials (ndev x RLC_PART_WORDS words)
    // concurrent verify batches (cc_set_concurrency): with K > 1 slots, cc_verify_batch_device /
    // cc_verify_batch_pervk_device / cc_pok_verify_batch_device / cc_pok_verify_batch_pervk_device /
    // cc_rlc_partial_device / cc_pok_rlc_partial_device calls take the
    // slots round-robin and are ordered only after the context's earlier work (tables, params) and the
    // same slot's previous batch, so K batches on K caller streams overlap (slots.h).  pool.recs[0] is
    // the context's own workspaces (prep / flags / fbuf / vkb / scratch / pok_idx / wide_*); vslots
    // holds the buffers of slots 1 .. K-1; stage[k] slot k's pinned upload ring.  Every other entry point
    // first waits for every slot's last batch.
    int concurrency = 1;
    HipDev dev;
    SlotPool pool;
    std::vector<VerifySlot*> vslots;
    std::vector<Staging> stage;
};

namespace cc {
namespace host __attribute__((visibility("hidden"))) {

// stream st waits (on the device) for every concurrent verify slot's last batch
static void wait_slots(cc_ctx* c, hipStream_t st) { c->pool.wait_all(c->dev, st); }
// the host waits for every concurrent verify slot's last batch (before buffers a slot may still read
// are freed or rebuilt: tables, params, workspaces)
static void drain_slots(cc_ctx* c) { c->pool.drain(c->dev); }

// Argument ceilings of the batch entry points (coconut_hip.h CC_MAX_BATCH etc.): every size product the
// host computes (n x q x 192 bytes, n x len x 8, grid dimensions) stays far inside size_t and the launch
// limits, so a garbage count is CC_ERR_DECODE before anything is allocated, copied or launched.
constexpr size_t kMaxBatch = CC_MAX_BATCH;  // credentials / proofs / points per call
constexpr size_t kMaxIds = CC_MAX_IDS;      // ids per credential (aggregation `len`)
constexpr size_t kMaxParts = CC_MAX_PARTS;  // gathered partials of one RLC finish
constexpr size_t kMaxQ = CC_MAX_Q;          // messages per credential (cc_set_verkey's bound)

// The next concurrent slot (round-robin, slots.h Pool): its workspaces grown to the batch's sizes once
// its last batch is done, and stream st ordered after the context stream's queued work (tables, params,
// other entry points) and after that last batch.  f(k, w) queues the batch on slot k's workspaces w; a
// SlotFence records the slot's completion on st on every exit.
template <class F>
static cc_status on_slot(cc_ctx* c, hipStream_t st, const cc::slots::Sizes& sz, F f) {
    const int k = c->pool.take();
    const VerifyWork w = c->pool.recs[(size_t)k].w;
    const int rc = c->pool.begin(c->dev, k, sz, st, c->stream, c->ev_order);
    if (rc) return rc == -2 ? CC_ERR_STATE : CC_ERR_HIP;
    SlotFence fence(c->pool, c->dev, k, st);
    const cc_status s = f(k, w);
    if (s) return s;
    return fence.close() ? CC_ERR_HIP : CC_OK;
}

static inline int sig_bytes(int mode) { return mode == 0 ? 192 : 97; }
static inline int oth_bytes(int mode) { return mode == 0 ? 97 : 192; }
static inline int oth_group(int mode) { return mode == 0 ? 1 : 2; }
static inline int sig_group(int mode) { return mode == 0 ? 2 : 1; }
static inline size_t aff_words(int group) { return group == 1 ? 24 : 48; }

// the context's own workspaces: concurrency slot 0, and every single-slot entry point
static VerifyWork ctx_work(cc_ctx* c) {
    return VerifyWork(&c->prep, &c->flags, &c->fbuf, &c->vkb, &c->scratch, &c->pok_idx, &c->wide_prep, &c->wide_flags,
                      &c->wide_f);
}

static inline cc_ctx* primary(cc_ctx* c) { return c && !c->peers.empty() ? c->peers[0] : c; }
static inline const cc_ctx* primary(const cc_ctx* c) { return c && !c->peers.empty() ? c->peers[0] : c; }

#define HIPCK(x) do { if ((x) != hipSuccess) return CC_ERR_HIP; } while (0)
#define KCK(x) do { if ((x) != 0) return CC_ERR_HIP; } while (0)

// the one-wave kernels' thresholds (slots.h, with the workspace sizes they decide; capi_verify.cpp)
using cc::slots::kFexpWideMax;
using cc::slots::kPrepWideMax;
using cc::slots::kWideMax;

// ---- helpers more than one area calls.  capi_ctx.cpp: decode / subgroup status of host encodings; the context's
// own workspaces (slot 0) grown to n credentials; the three phase times after a synchronise (cc_set_timing)
cc_status decode_points_host(cc_ctx* c, int group, size_t n, const uint8_t* bytes, uint32_t* d_out, uint32_t* d_inf);
cc_status subgroup_host(cc_ctx* c, int group, size_t n, const uint8_t* bytes, uint8_t* status);
cc_status ensure_work(cc_ctx* c, size_t n);
void collect_timing(cc_ctx* c);
// capi_verify.cpp: after a prep, the Miller loops and the final exponentiation; the RLC partial
cc_status launch_pairings(cc_ctx* c, const VerifyWork& w, size_t n, uint8_t* d_verdicts, uint8_t* d_gt, hipStream_t st);
int fresh_seed(uint8_t seed[32]);
// The RLC partial's workspaces: prep SoA (twin layout), flags, Miller values, the product tree's scratch,
// the delta key, the fall-back flag word, the fold points, delta digits and fold workspace.
struct RlcWork { DevBuf *prep, *flags, *fbuf, *scratch, *key, *any, *pts, *dig, *work; };
// The PoK form of the partial (pok_rlc.hip): part 1 is the PoK prep (Schnorr check, J's subgroup test,
// delta J') instead of the delta-scaled message MSM; its tables of d J live in the scratch, which the
// product tree takes over after the Miller loop.
struct PokRlcArgs {
    size_t r;
    const uint8_t *d_J, *d_T, *d_resp, *d_chal, *d_rev_msgs;
    const uint32_t* d_idx;
    bool twin;  // capi_pok.cpp pok_rlc_twin
};
RlcWork ctx_rlc_work(cc_ctx* c);
RlcWork slot_rlc_work(cc_ctx* c, int k);
int rlc_ensure(cc_ctx* c, const RlcWork& r, size_t n, SlotPool::Rec* sl, size_t scr_min = 0, bool twin = false);
cc_status launch_rlc_partial(cc_ctx* c, const RlcWork& w, size_t n, size_t q, uint64_t base_index, const uint8_t* seed32,
                             const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs, uint32_t* d_partial,
                             hipStream_t st, Staging* stage, const PokRlcArgs* pok = nullptr);
cc_status write_neutral_partial(uint32_t* d_partial, hipStream_t st);
// run f(k, lo, hi) for every peer k of a device set on its own host thread over the contiguous shard [lo, hi)
template <class F>
static cc_status for_shards(cc_ctx* c, size_t n, F f) {
    const size_t k = c->peers.size();
    std::vector<cc_status> st(k, CC_OK);
    std::vector<std::thread> th;
    for (size_t d = 0; d < k; d++)
        th.emplace_back([&, d] { st[d] = f(d, n * d / k, n * (d + 1) / k); });
    for (auto& t : th) t.join();
    for (cc_status s : st)
        if (s) return s;
    return CC_OK;
}
// The RLC host forms (cc_verify_batch, cc_pok_verify_batch_rlc) behind the uploads f has queued, as two
// sequences: partial(seed) queues the form's partial into c->rlc_part, then the finish and `accept` down,
// which ends f; only on reject (a bad element somewhere) a second one, each(g), takes the per-element launch
// and its downloads, so every verdict equals the reference's.
template <class Partial, class Each>
static cc_status rlc_host(cc_ctx* c, HostForm& f, size_t n, uint8_t* verdicts, Partial partial, Each each) {
    uint8_t seed[32], accept = 0;
    if (fresh_seed(seed)) return CC_ERR_HIP;
    if (c->rlc_part.ensure(RLC_PART_WORDS * 4) || c->rlc_accept.ensure(1)) return CC_ERR_HIP;
    f.launch([&]() -> cc_status {
        if (cc_status s = partial(seed)) return s;
        return cc_rlc_finish_device(c, 1, c->rlc_part.as<uint32_t>(), c->rlc_accept.as<uint8_t>(), nullptr, c->stream);
    });
    f.down(&accept, c->rlc_accept, 1);
    if (cc_status s = f.finish()) return s;
    if (accept) {
        memset(verdicts, 1, n);
        return CC_OK;
    }
    HostForm g(c->stream);
    return each(g);
}
// capi_pok.cpp: whether the PoK partial of n proofs takes the two-proof Miller loop (else the four-proof one)
bool pok_rlc_twin(cc_ctx* c, size_t n);
// capi_pok.cpp: the PoK forms' checks; capi_aggregate.cpp: the Straus scratch; capi_holder.cpp: the request forms' checks
cc_status prove_checks(const cc_ctx* c, bool with_vk, size_t q, size_t r, size_t nresp, const uint64_t* rev_idx,
                       std::vector<uint32_t>& idx);
cc_status agg_scratch(cc_ctx* c, int group, size_t ntask, size_t t);
cc_status rq_checks(const cc_ctx* c, bool with_params, size_t n, size_t q, size_t k);

}  // namespace host
}  // namespace cc

// Every *_device entry point may run on a caller stream while the context's workspaces (prep, flags,
// fbuf, scratch, RLC buffers, verkey tables) are shared with the host entry points, which run on
// c->stream.  StreamOrder makes the caller's stream wait for everything already queued on c->stream
// at entry, and c->stream wait for the call's work at exit, so calls on any mix of streams touch the
// workspaces in program order (two device calls on different streams are chained through c->stream).
// (outside cc::host, as before: its constructor and destructor are among the library's dynamic symbols)
struct StreamOrder {
    cc_ctx* c;
    hipStream_t st;
    StreamOrder(cc_ctx* c_, hipStream_t s) : c(c_), st(s) {
        wait_slots(c, st);
        if (st != c->stream) {
            (void)hipEventRecord(c->ev_order, c->stream);
            (void)hipStreamWaitEvent(st, c->ev_order, 0);
        }
    }
    ~StreamOrder() {
        if (st != c->stream) {
            (void)hipEventRecord(c->ev_order, st);
            (void)hipStreamWaitEvent(c->stream, c->ev_order, 0);
        }
    }
};
