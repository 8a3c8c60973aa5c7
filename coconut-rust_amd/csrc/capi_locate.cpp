// C ABI, RLC locate: the segmented partial (one RLC partial per segment of the batch, in one pass), the
// per-partial finish (one accept byte per partial), and the drivers that verify per credential only the
// segments whose own RLC check failed (locate_plan.h), so one bad credential costs a segment's
// re-verification instead of the batch's.  Single-slot calls: they drain the concurrency slots and are
// ordered on the context's stream like every entry point outside cc_set_concurrency's list.
#include "ctx.h"

namespace {

// the segmented form of launch_rlc_partial (capi_verify.cpp): the same prep, Miller launch and delta
// schedule over all n credentials, with the fall-back word, the fold and the product tree per segment
cc_status launch_rlc_partial_seg(cc_ctx* c, const RlcWork& w, size_t n, size_t q, size_t seg, uint64_t base_index,
                                 const uint8_t* seed32, const uint8_t* d_s1, const uint8_t* d_s2,
                                 const uint8_t* d_msgs, uint32_t* d_partials, hipStream_t st) {
    const size_t PS = (n + 1) / 2, N = (n + 3) / 4, S = cc::locate::segments(n, seg);
    const int segsh = cc::locate::log2_exact(seg);
    uint32_t* any = c->seg_any.as<uint32_t>();  // S words; word S takes the check kernels' batch-wide flag
    KCK(HipMem::h2d(w.key->p, seed32, 32, st));
    HIPCK(hipMemsetAsync(any, 0, (S + 1) * 4, st));
    auto prep_part = [&](int part) {
        return cck_prep_rlc(c->mode, part, n, PS, (int)q, base_index, w.key->as<uint32_t>(), d_s1, d_s2, d_msgs,
                            c->table.as<uint32_t>(), c->wbits, c->table_inf.as<uint32_t>(), w.prep->as<uint32_t>(),
                            w.flags->as<uint32_t>(), any + S, w.pts->as<uint32_t>(), w.dig->as<int8_t>(), st);
    };
    KCK(prep_part(0));
    KCK(cck_rlc_seg_flags(n, segsh, w.flags->as<uint32_t>(), any, st));
    // the fold per segment; its window sums (16 waves a segment) on the side stream beside the delta MSM
    KCK(cck_fold_seg(c->mode, n, seg, w.dig->as<int8_t>(), w.pts->as<uint32_t>(), c->seg_work.as<uint32_t>(), st));
    hipStream_t side = c->side ? c->side : st;
    if (side != st) {
        HIPCK(hipEventRecord(c->ev_fork, st));
        HIPCK(hipStreamWaitEvent(side, c->ev_fork, 0));
    }
    KCK(cck_fold_window_seg(c->mode, n, seg, c->seg_work.as<uint32_t>(), d_partials, side));
    KCK(prep_part(1));
    // SigG2: sigma_1's subgroup test from the loop's T raises the word of the credential's segment (four
    // credentials a loop, seg >= 4: a loop never straddles two segments); SigG1 tests sigma_1 in the check kernel
    KCK(c->mode == 0 ? cck_miller4_seg_lz_g2(n, PS, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                             w.fbuf->as<uint32_t>(), N, 0, any, segsh - 2, st)
                     : cck_miller4_lz_g1(n, PS, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                         w.fbuf->as<uint32_t>(), N, 0, nullptr, st));
    // the product tree down to the level of S values: value s is segment s's Miller product (seg = 4: level 0)
    KCK(cck_rlc_reduce_seg(N, S, w.fbuf->as<uint32_t>(), w.scratch->as<uint32_t>(), any, c->vk_subgroup ? 0u : 1u,
                           d_partials, st));
    if (side != st) {  // the window sections are part of the partials
        HIPCK(hipEventRecord(c->ev_join, side));
        HIPCK(hipStreamWaitEvent(st, c->ev_join, 0));
    }
    return CC_OK;
}

cc_status partial_seg_checks(const cc_ctx* c, size_t n, size_t q, size_t seg, const void* seed32, const void* d_s1,
                             const void* d_s2, const void* d_msgs, const void* d_out) {
    if (!c || !seed32 || (n && (!d_out || !d_s1 || !d_s2 || (q && !d_msgs)))) return CC_ERR_DECODE;
    if (n > kMaxBatch || !cc::locate::valid_seg(seg, kMaxBatch) || cc::locate::segments(n, seg) > kMaxParts)
        return CC_ERR_DECODE;
    if (!c->have_params || !c->have_vk) return CC_ERR_STATE;
    if (q != c->q) return CC_ERR_LEN;
    return CC_OK;
}

cc_status partial_seg(cc_ctx* c, size_t n, size_t q, size_t seg, uint64_t base_index, const uint8_t* seed32,
                      const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs, uint32_t* d_partials,
                      hipStream_t st) {
    const size_t S = cc::locate::segments(n, seg);
    drain_slots(c);  // concurrent batches (cc_set_concurrency) may still use the buffers sized below
    if (cc_status s = ensure_work(c, n)) return s;
    RlcWork r = ctx_rlc_work(c);
    if (rlc_ensure(c, r, n, nullptr) || c->seg_any.ensure((S + 1) * 4) ||
        c->seg_work.ensure(cck_fold_seg_words(c->mode, n, seg) * 4))
        return CC_ERR_HIP;
    StreamOrder order(c, st);
    return launch_rlc_partial_seg(c, r, n, q, seg, base_index, seed32, d_s1, d_s2, d_msgs, d_partials, st);
}

// the drivers' device form on one device: verdicts for credentials [0, n) with deltas base_index + i
cc_status locate_device(cc_ctx* c, size_t n, size_t q, size_t seg, uint64_t base_index, const uint8_t* seed32,
                        const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs, uint8_t* d_verdicts,
                        uint32_t* stats3, void* stream) {
    const size_t S = cc::locate::segments(n, seg), sb = (size_t)sig_bytes(c->mode);
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (c->loc_parts.ensure(S * RLC_PART_WORDS * 4) || c->loc_accept.ensure(S)) return CC_ERR_HIP;
    if (cc_status s = partial_seg(c, n, q, seg, base_index, seed32, d_s1, d_s2, d_msgs, c->loc_parts.as<uint32_t>(), st))
        return s;
    if (cc_status s = cc_rlc_finish_each_device(c, S, c->loc_parts.as<uint32_t>(), c->loc_accept.as<uint8_t>(), nullptr, st))
        return s;
    std::vector<uint8_t> accept(S, 0);
    KCK(HipMem::d2h(accept.data(), c->loc_accept.p, S, st));
    KCK(HipMem::sync(st));  // the one synchronisation: the accept bytes decide what is launched next
    const cc::locate::Plan p = cc::locate::plan(n, seg, accept.data());
    if (stats3) stats3[0] = (uint32_t)p.segments, stats3[1] = (uint32_t)p.rejected, stats3[2] = (uint32_t)p.rechecked;
    if (p.in_place())  // nothing to skip: per credential where the batch lies
        return cc_verify_batch_device(c, n, q, d_s1, d_s2, d_msgs, d_verdicts, nullptr, st);
    HIPCK(hipMemsetAsync(d_verdicts, 1, n, st));  // every credential of an accepted segment verifies
    if (!p.rechecked) return CC_OK;
    // the rejected runs' rows side by side, ONE per-credential launch sequence over them, verdicts back
    const size_t m = p.rechecked;
    if (c->loc_s1.ensure(m * sb) || c->loc_s2.ensure(m * sb) || c->loc_msgs.ensure(m * q * 48 + 16) ||
        c->loc_verdicts.ensure(m))
        return CC_ERR_HIP;
    auto d2d = [&](void* d, const void* s, size_t bytes) {
        return bytes ? hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
    };
    for (const cc::locate::Run& r : p.runs) {
        const size_t len = r.hi - r.lo;
        HIPCK(d2d(c->loc_s1.as<uint8_t>() + r.off * sb, d_s1 + r.lo * sb, len * sb));
        HIPCK(d2d(c->loc_s2.as<uint8_t>() + r.off * sb, d_s2 + r.lo * sb, len * sb));
        HIPCK(d2d(c->loc_msgs.as<uint8_t>() + r.off * q * 48, d_msgs + r.lo * q * 48, len * q * 48));
    }
    if (cc_status s = cc_verify_batch_device(c, m, q, c->loc_s1.as<uint8_t>(), c->loc_s2.as<uint8_t>(),
                                             c->loc_msgs.as<uint8_t>(), c->loc_verdicts.as<uint8_t>(), nullptr, st))
        return s;
    for (const cc::locate::Run& r : p.runs)
        HIPCK(d2d(d_verdicts + r.lo, c->loc_verdicts.as<uint8_t>() + r.off, r.hi - r.lo));
    return CC_OK;
}

}  // namespace

cc_status cc_rlc_partial_seg_device(cc_ctx* c, size_t n, size_t q, size_t seg, uint64_t base_index,
                                    const uint8_t* seed32, const uint8_t* d_s1, const uint8_t* d_s2,
                                    const uint8_t* d_msgs, uint32_t* d_partials, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (cc_status s = partial_seg_checks(c, n, q, seg, seed32, d_s1, d_s2, d_msgs, d_partials)) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    return partial_seg(c, n, q, seg, base_index, seed32, d_s1, d_s2, d_msgs, d_partials,
                       stream ? (hipStream_t)stream : c->stream);
}

cc_status cc_rlc_finish_each_device(cc_ctx* c, size_t nparts, const uint32_t* d_partials, uint8_t* d_accept,
                                    uint8_t* d_gt, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !nparts || nparts > kMaxParts || !d_partials || !d_accept) return CC_ERR_DECODE;
    if (!c->have_params || !c->have_vk) return CC_ERR_STATE;  // the window pairs' P_w come with the verkey
    HIPCK(hipSetDevice(c->device));
    // cc_rlc_finish_device's buffers and ordering (ev_fin: finishes of either kind run in call order, and a
    // verkey change waits for the last one).  fin_f: the 16 k window values, then k_fexp1's chain;
    // fin_scratch: the tree's other half, then the k products
    const size_t k = nparts, NW = (size_t)RLC_WINDOWS * k;
    if (c->fin_each_flags.ensure(k * 4) ||
        c->fin_f.ensure(std::max(NW * 144 * 4, std::min(k, kFexpWideMax) * 72 * 12 * 4)) ||
        c->fin_scratch.ensure((NW / 2) * 144 * 4) || c->fin_prep.ensure((size_t)PREP_SLOTS * 12 * NW * 4) ||
        c->fin_flags2.ensure(NW * 4))
        return CC_ERR_HIP;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (c->fin_recorded) HIPCK(hipStreamWaitEvent(st, c->ev_fin, 0));
    KCK(cck_rlc_gather_each(c->mode, k, d_partials, c->rlc_pw.as<uint32_t>(), c->rlc_finf.as<uint8_t>(),
                            c->fin_prep.as<uint32_t>(), c->fin_flags2.as<uint32_t>(),
                            c->fin_each_flags.as<uint32_t>(), st));
    KCK(cck_miller_wide(NW, c->fin_prep.as<uint32_t>(), c->fin_flags2.as<uint32_t>(), c->fin_f.as<uint32_t>(), NW, 0,
                        st));
    KCK(cck_rlc_each_products(k, c->fin_f.as<uint32_t>(), c->fin_scratch.as<uint32_t>(), d_partials, st));
    KCK(cck_fexp(k, c->fin_scratch.as<uint32_t>(), c->fin_f.as<uint32_t>(), c->fin_each_flags.as<uint32_t>(), d_accept,
                 d_gt, kFexpWideMax, st));
    HIPCK(hipEventRecord(c->ev_fin, st));
    c->fin_recorded = true;
    return CC_OK;
}

cc_status cc_verify_batch_locate_device(cc_ctx* c, size_t n, size_t q, size_t seg, const uint8_t* seed32,
                                        const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs,
                                        uint8_t* d_verdicts, uint32_t* stats3, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!seg && c) seg = cc::locate::default_seg(c->mode);
    if (cc_status s = partial_seg_checks(c, n, q, seg, seed32, d_s1, d_s2, d_msgs, d_verdicts)) return s;
    if (stats3) stats3[0] = stats3[1] = stats3[2] = 0;
    if (!n) return CC_OK;
    return locate_device(c, n, q, seg, 0, seed32, d_s1, d_s2, d_msgs, d_verdicts, stats3, stream);
}

cc_status cc_verify_batch_locate(cc_ctx* c, size_t n, size_t q, size_t seg, const uint8_t* s1, const uint8_t* s2,
                                 const uint8_t* msgs, uint8_t* verdicts, uint32_t* stats3) {
    if (!seg && c) seg = cc::locate::default_seg(primary(c)->mode);
    uint8_t seed[32] = {0};
    if (cc_status s = partial_seg_checks(primary(c), n, q, seg, seed, s1, s2, msgs, verdicts)) return s;
    if (stats3) stats3[0] = stats3[1] = stats3[2] = 0;
    if (!n) return CC_OK;
    if (fresh_seed(seed)) return CC_ERR_HIP;
    // one device's share: rows [lo, lo + m) staged into its input buffers, located with deltas lo + i
    auto shard = [&](cc_ctx* p, size_t lo, size_t m, uint32_t* st3) -> cc_status {
        const size_t sb = (size_t)sig_bytes(p->mode);
        HIPCK(hipSetDevice(p->device));
        drain_slots(p);  // concurrent device batches may still read the input buffers
        if (p->in_s1.ensure(m * sb) || p->in_s2.ensure(m * sb) || p->in_msgs.ensure(m * q * 48 + 16) ||
            p->verdicts.ensure(m))
            return CC_ERR_HIP;
        HostForm f(p->stream);
        f.up(p->in_s1, s1 + lo * sb, m * sb);
        f.up(p->in_s2, s2 + lo * sb, m * sb);
        f.up(p->in_msgs, msgs + lo * q * 48, m * q * 48);
        f.launch([&] {
            return locate_device(p, m, q, seg, lo, seed, p->in_s1.as<uint8_t>(), p->in_s2.as<uint8_t>(),
                                 p->in_msgs.as<uint8_t>(), p->verdicts.as<uint8_t>(), st3, p->stream);
        });
        f.down(verdicts + lo, p->verdicts, m);
        return f.finish();
    };
    if (c->peers.empty()) return shard(c, 0, n, stats3);
    // a device set: every device locates inside its own shard; no collective
    std::vector<uint32_t> st3(3 * c->peers.size(), 0);
    cc_status s = for_shards(c, n, [&](size_t d, size_t lo, size_t hi) -> cc_status {
        return hi == lo ? CC_OK : shard(c->peers[d], lo, hi - lo, &st3[3 * d]);
    });
    if (s) return s;
    if (stats3)
        for (size_t d = 0; d < c->peers.size(); d++)
            for (int j = 0; j < 3; j++) stats3[j] += st3[3 * d + j];
    return CC_OK;
}
