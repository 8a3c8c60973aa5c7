// C ABI, contexts and tables: status and version strings, cc_ctx_create / destroy and the device sets, timing,
// concurrency slots, cc_device_error, params, verkey and the shared-verkey tables (ctx.h).
#include "ctx.h"

// default HBM budget of a context's shared-verkey tables (wider: cc_set_table_bits)
constexpr double kVkTableBudget = 4.0 * (double)(1ull << 30);

// free HBM of the current device (0 if the runtime cannot say)
size_t cc::host::free_hbm() {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return fr;
}

cc_status cc::host::decode_points_host(cc_ctx* c, int group, size_t n, const uint8_t* bytes, uint32_t* d_out,
                                       uint32_t* d_inf) {
    size_t eb = group == 1 ? 97 : 192;
    DevBuf tmp;
    if (tmp.ensure(eb * n + 16)) return CC_ERR_HIP;
    HostForm f(c->stream);
    f.up(tmp, bytes, eb * n);
    f.launch([&] { return cck_decode_points(group, n, tmp.as<uint8_t>(), d_out, d_inf, c->stream); });
    return f.finish();
}

cc_status cc::host::subgroup_host(cc_ctx* c, int group, size_t n, const uint8_t* bytes, uint8_t* status) {
    size_t eb = group == 1 ? 97 : 192;
    DevBuf tmp, st;
    if (tmp.ensure(eb * n + 16) || st.ensure(n + 16)) return CC_ERR_HIP;
    HostForm f(c->stream);
    f.up(tmp, bytes, eb * n);
    f.launch([&] { return cck_subgroup(group, n, tmp.as<uint8_t>(), st.as<uint8_t>(), c->stream); });
    f.down(status, st, n);
    return f.finish();
}

// the context's own workspaces (slot 0) grown to n credentials; scratch: the PoK prep's per-proof table
// of d J (15 Jacobian points, <= 15 x 84 words: SigG1's lazy G2 points), and the one-wave fexp's
// (fexp_pl.hip k_fexp1: 72 slots of 12 words an element); the batched fexp (fexp_q.hip) keeps its chain
// in registers
cc_status cc::host::ensure_work(cc_ctx* c, size_t n) {
    const cc::slots::Sizes sz = cc::slots::verify_sizes(n, 0, (n * 15 * 84 + 72 * 12) * 4, 0);
    const VerifyWork w = ctx_work(c);
    if (w.short_of(sz) || c->verdicts.bytes < n)
        drain_slots(c);  // a concurrent batch may still read the buffers about to be reallocated
    for (int j = 0; j < VerifyWork::kN; j++)
        if (w.at(j)->ensure(sz.at(j))) return CC_ERR_HIP;
    if (c->verdicts.ensure(n)) return CC_ERR_HIP;
    return CC_OK;
}

void cc::host::collect_timing(cc_ctx* c) {
    if (!c->timing) return;
    (void)hipEventSynchronize(c->ev[3]);
    for (int k = 0; k < 3; k++) (void)hipEventElapsedTime(&c->last_ms[k], c->ev[k], c->ev[k + 1]);
}

// Shared-verkey tables: by default the widest of 22 / 20 / 18 / 16 / 14 / 12 / 10-bit windows whose q + 2
// bases' tables fit kVkTableBudget (4 GiB) and 40 % of the free HBM — a drop-in verifier must not claim a
// shared GPU's memory: config 2 (q = 6, 8 G1 bases) gets 18 bits (15 windows of 262,143 entries, 3.0 GB),
// config 3 (q = 16) 16 bits (1.8 GB); 16 / 15 / 12 mixed additions per scalar at 16 / 18 / 22 bits.  Wider
// tables (22 bits: 4.8 / 9.7 GB a G1 / G2 base, +1.2 % on config 2, profiles/r03/vkbits) are opt-in through
// cc_set_table_bits, which forces a width in [8, 22]; else 8-bit windows (32 x 255 entries, 0.8 / 1.6 MB a
// base); a failed wide allocation falls back to 8 bits.  On failure the caller leaves the context without
// a verkey.
static cc_status rebuild_tables(cc_ctx* c) {
    // bases for the fixed-base tables: Y~[0..q), g~ (PoK Schnorr base), X~ (RLC) -> q + 2 bases
    int og = oth_group(c->mode);
    size_t aw = aff_words(og);
    int nb = (int)c->q + 2;
    int wb = c->force_vk_bits;
    auto tbytes = [&](int w) { return (size_t)nb * tab_words(og, w) * 4; };
    // the old table is released first so its memory counts as free
    c->table.release();
    if (!wb) {
        const double cap = std::min(0.4 * (double)free_hbm(), kVkTableBudget);
        wb = 8;
        for (int w : {22, 20, 18, 16, 14, 12, 10})
            if ((double)tbytes(w) <= cap) {
                wb = w;
                break;
            }
    }
    wb = alloc_tables(wb, c->force_vk_bits != 0, tbytes, [&](int w) { return c->table.ensure(tbytes(w)) == 0; });
    if (!wb) return CC_ERR_HIP;
    c->wbits = wb;
    c->vk_built_force = c->force_vk_bits;
    if (c->table_inf.ensure((size_t)nb * 4)) return CC_ERR_HIP;
    // [Y~..., g~, X~] are contiguous in vk_aff (X~ at 0, Y~ at 1..q, g~ at q+1, X~ again at q+2)
    HIPCK(hipMemcpyAsync(c->table_inf.p, c->vk_inf.as<uint32_t>() + 1, (size_t)nb * 4, hipMemcpyDeviceToDevice,
                         c->stream));
    DevBuf pw;
    if (pw.ensure((size_t)nb * tab_nwin(c->wbits) * (og == 1 ? 36 : 72) * 4)) return CC_ERR_HIP;
    KCK(cck_build_table(og, nb, c->wbits, c->vk_aff.as<uint32_t>() + aw, c->table_inf.as<uint32_t>(), pw.as<uint32_t>(),
                        c->table.as<uint32_t>(), 1, c->stream));
    // the RLC window pairs' fixed points P_w = (256^w) g~ (g~ = base q); an RLC finish still running on
    // another stream reads them, so the rewrite waits for it
    if (c->rlc_pw.ensure((size_t)PREP_SLOTS * 12 * RLC_WINDOWS * 4) || c->rlc_finf.ensure(RLC_WINDOWS))
        return CC_ERR_HIP;
    if (c->fin_recorded) HIPCK(hipStreamWaitEvent(c->stream, c->ev_fin, 0));
    KCK(cck_fold_fixed(c->mode, (int)c->q, c->table.as<uint32_t>(), c->wbits, c->table_inf.as<uint32_t>(),
                       c->rlc_pw.as<uint32_t>(), c->rlc_finf.as<uint8_t>(), c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return CC_OK;
}

// subgroup status of the verkey points (X~ || Y~, q + 1 encodings) and the context's g~: the RLC accepts
// only when all are in the order-r subgroup.  Depends on g~ as well, so cc_set_params recomputes it
// whenever it rebinds g~ under an existing verkey.
static cc_status refresh_vk_subgroup(cc_ctx* c, const uint8_t* vk_all, size_t q) {
    c->vk_subgroup = false;
    const int og = oth_group(c->mode);
    std::vector<uint8_t> st(q + 1);
    cc_status s = subgroup_host(c, og, q + 1, vk_all, st.data());
    if (s) return s;
    uint8_t gst = 0;
    s = subgroup_host(c, og, 1, c->gtilde_bytes.data(), &gst);
    if (s) return s;
    bool ok = gst == 2;
    for (size_t k = 0; k <= q; k++) ok = ok && st[k] == 2;
    c->vk_subgroup = ok;
    return CC_OK;
}

const char* cc_status_str(int s) {
    switch (s) {
        case CC_OK: return "ok";
        case CC_ERR_LEN: return "UnsupportedNoOfMessages";
        case CC_ERR_BASES_EXPS: return "UnequalNoOfBasesExponents";
        case CC_ERR_THRESHOLD: return "fewer entries than threshold";
        case CC_ERR_DECODE: return "bad buffer / size";
        case CC_ERR_HIP: return "HIP runtime error";
        case CC_ERR_RCCL: return "RCCL error";
        case CC_ERR_STATE: return "params/verkey not set";
        default: return "unknown";
    }
}

// CC_SRC_HASH: tools/src_hash.py over csrc/, the header, the Makefile and the flags (Makefile)
#ifndef CC_SRC_HASH
#define CC_SRC_HASH "unknown"
#endif
const char* cc_version(void) { return "coconut-mi355x 0.2.0 (gfx950) src " CC_SRC_HASH; }

static_assert(CC_RLC_PARTIAL_WORDS == RLC_PART_WORDS, "coconut_hip.h and rlc_part.h disagree");
int cc_rlc_partial_words(void) { return RLC_PART_WORDS; }

cc_status cc_ctx_create(int device, cc_group_mode mode, cc_ctx** out) {
    if (!out || (mode != CC_SIG_G2 && mode != CC_SIG_G1)) return CC_ERR_DECODE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return CC_ERR_HIP;
    HIPCK(hipSetDevice(device));
    cc_ctx* c = new cc_ctx();
    c->device = device;
    c->mode = (int)mode;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return CC_ERR_HIP;
    }
    for (auto& e : c->ev) (void)hipEventCreate(&e);
    (void)hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&c->ev_fin, hipEventDisableTiming);
    {
        // high priority: a launch on the side stream gets its wave slots before a full launch on the
        // context stream fills the chip
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, hi) != hipSuccess) c->side = nullptr;
    }
    c->pool.recs.resize(1);
    c->pool.recs[0].w = ctx_work(c);  // slot 0: the context's own workspaces
    c->stage.resize(1);
    *out = c;
    return CC_OK;
}

cc_status cc_ctx_destroy(cc_ctx* c) {
    if (!c) return CC_OK;
    if (!c->peers.empty()) {
        for (size_t k = 0; k < c->comms.size(); k++) {
            (void)hipSetDevice(c->peers[k]->device);
            ncclCommDestroy(c->comms[k]);
        }
        for (cc_ctx* p : c->peers) cc_ctx_destroy(p);
        delete c;
        return CC_OK;
    }
    (void)hipSetDevice(c->device);
    drain_slots(c);
    (void)hipStreamSynchronize(c->stream);
    for (VerifySlot* v : c->vslots) delete v;
    c->vslots.clear();
    for (auto& r : c->pool.recs)
        if (r.done) (void)hipEventDestroy(r.done);
    c->pool.recs.clear();
    for (Staging& g : c->stage) g.release(c->dev);
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_fin) (void)hipEventDestroy(c->ev_fin);
    if (c->side) (void)hipStreamDestroy(c->side);
    (void)hipStreamDestroy(c->stream);
    delete c;  // frees every device buffer the context owns (DevBuf)
    return CC_OK;
}

cc_status cc_ctx_mode(const cc_ctx* c, int* m) {
    if (!c || !m) return CC_ERR_DECODE;
    *m = c->mode;
    return CC_OK;
}

cc_status cc_set_timing(cc_ctx* c, int enabled) {
    c = primary(c);  // a device set forwards to its first device
    if (!c) return CC_ERR_DECODE;
    c->timing = enabled != 0;
    return CC_OK;
}

cc_status cc_last_timing(const cc_ctx* c, float* a, float* b, float* d) {
    c = primary(c);  // a device set forwards to its first device
    if (!c) return CC_ERR_DECODE;
    if (a) *a = c->last_ms[0];
    if (b) *b = c->last_ms[1];
    if (d) *d = c->last_ms[2];
    return CC_OK;
}

cc_status cc_set_params(cc_ctx* c, const uint8_t* g_tilde) {
    if (!c || !g_tilde) return CC_ERR_DECODE;
    if (!c->peers.empty()) {
        for (cc_ctx* p : c->peers) {
            cc_status s = cc_set_params(p, g_tilde);
            if (s) return s;
        }
        c->have_params = true;
        return CC_OK;
    }
    // the same g~ again (a caller re-binding its Params every batch): nothing to do
    if (c->have_params && c->gtilde_bytes.size() == (size_t)oth_bytes(c->mode) &&
        !memcmp(c->gtilde_bytes.data(), g_tilde, c->gtilde_bytes.size()))
        return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent verify batches read g~ and the tables rebuilt below
    c->have_params = false;  // until the decode below has succeeded
    c->gtilde_bytes.clear();
    int og = oth_group(c->mode);
    size_t aw = aff_words(og);
    if (c->gtilde_aff.ensure(aw * 4)) return CC_ERR_HIP;
    DevBuf inf;
    if (inf.ensure(4)) return CC_ERR_HIP;
    cc_status s = decode_points_host(c, og, 1, g_tilde, c->gtilde_aff.as<uint32_t>(), inf.as<uint32_t>());
    if (s) return s;
    HIPCK(hipMemcpy(&c->gtilde_inf, inf.p, 4, hipMemcpyDeviceToHost));
    c->gtilde_bytes.assign(g_tilde, g_tilde + oth_bytes(c->mode));
    if (c->mode == 1) {
        if (c->gtilde_lines.ensure(68 * 72 * 4)) return CC_ERR_HIP;
        KCK(cck_gtilde_lines(c->gtilde_aff.as<uint32_t>(), c->gtilde_lines.as<uint32_t>(), c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    } else {
        if (c->gtilde_lz.ensure(aw * 4)) return CC_ERR_HIP;
        KCK(cck_lazy_form(2, c->gtilde_aff.as<uint32_t>(), c->gtilde_lz.as<uint32_t>(), c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    }
    c->have_params = true;
    if (c->have_vk) {
        // refresh g~ slot of the verkey block and its table
        HIPCK(hipMemcpy(c->vk_aff.as<uint32_t>() + (c->q + 1) * aw, c->gtilde_aff.p, aw * 4, hipMemcpyDeviceToDevice));
        HIPCK(hipMemcpy(c->vk_inf.as<uint32_t>() + (c->q + 1), &c->gtilde_inf, 4, hipMemcpyHostToDevice));
        cc_status st = refresh_vk_subgroup(c, c->vk_bytes.data(), c->q);
        if (!st) st = rebuild_tables(c);
        if (st) {
            c->have_vk = false;
            c->q = 0;
            c->vk_bytes.clear();
        }
        return st;
    }
    return CC_OK;
}

cc_status cc_set_verkey(cc_ctx* c, const uint8_t* X, const uint8_t* Y, size_t q) {
    if (!c || !X || (q && !Y) || q > 4096) return CC_ERR_DECODE;
    if (!c->have_params) return CC_ERR_STATE;
    if (!c->peers.empty()) {
        c->have_vk = false;
        c->q = 0;
        for (cc_ctx* p : c->peers) {
            cc_status s = cc_set_verkey(p, X, Y, q);
            if (s) return s;
        }
        c->q = q;
        c->have_vk = true;
        return CC_OK;
    }
    int og = oth_group(c->mode);
    size_t eb = (size_t)oth_bytes(c->mode), aw = aff_words(og);
    std::vector<uint8_t> all((q + 1) * eb);
    memcpy(all.data(), X, eb);
    if (q) memcpy(all.data() + eb, Y, q * eb);
    // the same verkey again, tables built at the width now asked for: nothing to rebuild (a caller
    // binding its verkey every batch, INTEGRATION.md §3, pays a byte compare, not a table build)
    if (c->have_vk && c->q == q && c->vk_built_force == c->force_vk_bits && c->vk_bytes == all) return CC_OK;
    // no verkey until every step below has succeeded: a failed call leaves the context refusing
    // verify / RLC / PoK calls with CC_ERR_STATE instead of running on a half-built table
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent verify batches read the verkey and its tables
    c->have_vk = false;
    c->q = 0;
    c->vk_bytes.clear();
    if (c->vk_aff.ensure((q + 3) * aw * 4) || c->vk_inf.ensure((q + 3) * 4)) return CC_ERR_HIP;
    cc_status s = decode_points_host(c, og, q + 1, all.data(), c->vk_aff.as<uint32_t>(), c->vk_inf.as<uint32_t>());
    if (s) return s;
    HIPCK(hipMemcpy(c->vk_aff.as<uint32_t>() + (q + 1) * aw, c->gtilde_aff.p, aw * 4, hipMemcpyDeviceToDevice));
    HIPCK(hipMemcpy(c->vk_inf.as<uint32_t>() + (q + 1), &c->gtilde_inf, 4, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->vk_aff.as<uint32_t>() + (q + 2) * aw, c->vk_aff.p, aw * 4, hipMemcpyDeviceToDevice));
    HIPCK(hipMemcpy(c->vk_inf.as<uint32_t>() + (q + 2), c->vk_inf.p, 4, hipMemcpyDeviceToDevice));
    HIPCK(hipMemcpy(&c->X_inf, c->vk_inf.p, 4, hipMemcpyDeviceToHost));
    {
        cc_status s2 = refresh_vk_subgroup(c, all.data(), q);
        if (s2) return s2;
    }
    c->q = q;
    cc_status st = rebuild_tables(c);
    if (st) {
        c->q = 0;
        return st;
    }
    c->vk_bytes.swap(all);
    c->have_vk = true;
    return CC_OK;
}

cc_status cc_set_table_bits(cc_ctx* c, int verkey_bits, int issuer_bits) {
    if (!c || (verkey_bits != 0 && (verkey_bits < 8 || verkey_bits > 22)) ||
        (issuer_bits != 0 && (issuer_bits < 8 || issuer_bits > 16)))
        return CC_ERR_DECODE;
    for (cc_ctx* p : c->peers) {
        p->force_vk_bits = verkey_bits;
        p->force_iss_bits = issuer_bits;
    }
    c->force_vk_bits = verkey_bits;
    c->force_iss_bits = issuer_bits;
    return CC_OK;
}

cc_status cc_table_bits(const cc_ctx* c, int* verkey_bits, int* issuer_bits) {
    c = primary(c);
    if (!c) return CC_ERR_DECODE;
    if (verkey_bits) *verkey_bits = c->have_vk ? c->wbits : 0;
    if (issuer_bits) *issuer_bits = c->iss_n ? c->iss_wbits : 0;
    return CC_OK;
}

cc_status cc_set_concurrency(cc_ctx* c, int slots) {
    if (!c || slots < 1 || slots > 8) return CC_ERR_DECODE;
    for (cc_ctx* p : c->peers) {
        cc_status s = cc_set_concurrency(p, slots);
        if (s) return s;
    }
    if (!c->peers.empty()) {
        c->concurrency = slots;
        return CC_OK;
    }
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);
    while ((int)c->vslots.size() > slots - 1) {
        VerifySlot* v = c->vslots.back();
        c->vslots.pop_back();
        delete v;
        if (c->pool.recs.back().done) (void)hipEventDestroy(c->pool.recs.back().done);
        c->pool.recs.pop_back();
        c->stage.back().release(c->dev);
        c->stage.pop_back();
    }
    if (!c->pool.recs[0].done) HIPCK(hipEventCreateWithFlags(&c->pool.recs[0].done, hipEventDisableTiming));
    while ((int)c->vslots.size() < slots - 1) {
        SlotPool::Rec r;
        if (hipEventCreateWithFlags(&r.done, hipEventDisableTiming) != hipSuccess) return CC_ERR_HIP;
        VerifySlot* v = new VerifySlot;
        r.w = v->work();
        c->vslots.push_back(v);
        c->pool.recs.push_back(r);
        c->stage.emplace_back();
    }
    c->concurrency = slots;
    c->pool.next = 0;
    return CC_OK;
}

cc_status cc_concurrency(const cc_ctx* c, int* slots) {
    if (!c || !slots) return CC_ERR_DECODE;
    *slots = c->concurrency;
    return CC_OK;
}

cc_status cc_device_error(cc_ctx* c, void* stream, uint32_t* out) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !out) return CC_ERR_DECODE;
    *out = 0;
    if (!c->dev_err.p) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    uint32_t v = 0;
    HIPCK(hipMemcpyAsync(&v, c->dev_err.p, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemsetAsync(c->dev_err.p, 0, 4, st));
    HIPCK(hipStreamSynchronize(st));
    *out = v;
    return CC_OK;
}

// ---------------------------------------------------------------- device sets + RCCL (SURVEY.md §8b/§8e;
// the sharded verify: capi_verify.cpp multi_verify)
cc_status cc_ctx_create_multi(uint64_t device_mask, cc_group_mode mode, cc_ctx** out) {
    if (!out || !device_mask || (mode != CC_SIG_G2 && mode != CC_SIG_G1)) return CC_ERR_DECODE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return CC_ERR_HIP;
    std::vector<int> devs;
    for (int d = 0; d < 64; d++)
        if ((device_mask >> d) & 1ull) {
            if (d >= ndev) return CC_ERR_HIP;
            devs.push_back(d);
        }
    cc_ctx* c = new cc_ctx();
    c->device = devs[0];
    c->mode = (int)mode;
    for (int d : devs) {
        cc_ctx* p = nullptr;
        cc_status s = cc_ctx_create(d, mode, &p);
        if (s) {
            for (cc_ctx* q : c->peers) cc_ctx_destroy(q);
            delete c;
            return s;
        }
        c->peers.push_back(p);
    }
    c->comms.resize(devs.size());
    if (ncclCommInitAll(c->comms.data(), (int)devs.size(), devs.data()) != ncclSuccess) {
        c->comms.clear();
        for (cc_ctx* q : c->peers) cc_ctx_destroy(q);
        delete c;
        return CC_ERR_RCCL;
    }
    *out = c;
    return CC_OK;
}

cc_status cc_ctx_num_devices(const cc_ctx* c, int* n) {
    if (!c || !n) return CC_ERR_DECODE;
    *n = c->peers.empty() ? 1 : (int)c->peers.size();
    return CC_OK;
}
