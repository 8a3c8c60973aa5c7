// C ABI, RLC locate for PoKOfSignatureProof::verify: the segmented PoK partial (one RLC partial per segment
// of the batch, in one pass) and the drivers that verify per proof only the segments whose own RLC check
// failed.  The partial format, the segmented fold and product tree, the per-partial finish
// (cc_rlc_finish_each_device) and the plan (locate_plan.h) are capi_locate.cpp's; here are the PoK prep's
// per-segment fall-back words, the segmented two-proof Miller launch and the compaction of the seven
// per-proof arrays.  Single-slot calls, as the signature locate calls are.
#include "ctx.h"

namespace {

struct PokArrays {
    const uint8_t *s1, *s2, *J, *T, *resp, *chal, *rev;
};

// the segmented form of launch_rlc_partial's PoK branch (capi_verify.cpp): the same preps, Miller launch and
// delta schedule over all n proofs, with the fall-back word, the fold and the product tree per segment
cc_status launch_pok_partial_seg(cc_ctx* c, const RlcWork& w, size_t n, size_t q, size_t r, size_t seg, bool twin,
                                 uint64_t base_index, const uint8_t* seed32, const PokArrays& a, const uint32_t* d_idx,
                                 uint32_t* d_partials, hipStream_t st) {
    const size_t PS = (n + 1) / 2, N = twin ? PS : (n + 3) / 4, S = cc::locate::segments(n, seg);
    const int segsh = cc::locate::log2_exact(seg);
    uint32_t* any = c->seg_any.as<uint32_t>();  // S words; word S takes the prep kernels' batch-wide flag
    KCK(HipMem::h2d(w.key->p, seed32, 32, st));
    HIPCK(hipMemsetAsync(any, 0, (S + 1) * 4, st));
    KCK(cck_prep_rlc(c->mode, 0, n, PS, (int)q, base_index, w.key->as<uint32_t>(), a.s1, a.s2, nullptr,
                     c->table.as<uint32_t>(), c->wbits, c->table_inf.as<uint32_t>(), w.prep->as<uint32_t>(),
                     w.flags->as<uint32_t>(), any + S, w.pts->as<uint32_t>(), w.dig->as<int8_t>(), st));
    // the fold per segment; its window sums (16 waves a segment) on the side stream beside the PoK prep
    KCK(cck_fold_seg(c->mode, n, seg, w.dig->as<int8_t>(), w.pts->as<uint32_t>(), c->seg_work.as<uint32_t>(), st));
    hipStream_t side = c->side ? c->side : st;
    if (side != st) {
        HIPCK(hipEventRecord(c->ev_fork, st));
        HIPCK(hipStreamWaitEvent(side, c->ev_fork, 0));
    }
    KCK(cck_fold_window_seg(c->mode, n, seg, c->seg_work.as<uint32_t>(), d_partials, side));
    // Schnorr check, J's subgroup test, delta J'; the tables of d J in the scratch, which the product tree
    // takes over after the Miller loop.  The prep's own word is the spare one: a proof's flag bits raise its
    // segment's word (both preps' bits in one pass)
    KCK(cck_prep_pok_rlc(c->mode, n, PS, (int)q, (int)r, base_index, w.key->as<uint32_t>(), a.J, a.T, a.resp, a.chal,
                         a.rev, d_idx, c->table.as<uint32_t>(), c->wbits, c->table_inf.as<uint32_t>(),
                         w.prep->as<uint32_t>(), w.flags->as<uint32_t>(), any + S, w.scratch->as<uint32_t>(), st));
    KCK(cck_rlc_seg_flags_pok(n, segsh, w.flags->as<uint32_t>(), any, st));
    bool joined = false;
    if (twin && side != st) {  // one wave a SIMD needs every CU free when the loop's blocks are placed
        HIPCK(hipEventRecord(c->ev_join, side));
        HIPCK(hipStreamWaitEvent(st, c->ev_join, 0));
        joined = true;
    }
    // SigG2: sigma'_1's subgroup test from the loop's T raises the word of the proof's segment (two proofs a
    // loop and seg >= 4, four beyond the twin limit: a loop never straddles two segments)
    uint32_t *prep = w.prep->as<uint32_t>(), *flags = w.flags->as<uint32_t>(), *fbuf = w.fbuf->as<uint32_t>();
    if (twin)
        KCK(c->mode == 0 ? cck_miller_twin_seg_lz_g2(n, PS, prep, flags, fbuf, N, 0, any, segsh - 1, st)
                         : cck_miller_lz_g1(1, n, PS, prep, flags, c->gtilde_lines.as<uint32_t>(), fbuf, N, 0, nullptr,
                                            st));
    else
        KCK(c->mode == 0 ? cck_miller4_seg_lz_g2(n, PS, prep, flags, fbuf, N, 0, any, segsh - 2, st)
                         : cck_miller4_lz_g1(n, PS, prep, flags, fbuf, N, 0, nullptr, st));
    // the product tree down to the level of S values: value s is segment s's Miller product
    KCK(cck_rlc_reduce_seg(N, S, fbuf, w.scratch->as<uint32_t>(), any, c->vk_subgroup ? 0u : 1u, d_partials, st));
    if (side != st && !joined) {  // the window sections are part of the partials
        HIPCK(hipEventRecord(c->ev_join, side));
        HIPCK(hipStreamWaitEvent(st, c->ev_join, 0));
    }
    return CC_OK;
}

// cc_pok_rlc_partial_device's checks in its order (d_out: the partials, or the drivers' verdicts; both only
// read when n > 0), then cc_rlc_partial_seg_device's for seg and S
cc_status pok_seg_checks(const cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, size_t seg, const void* seed32,
                         const PokArrays& a, const uint64_t* rev_idx, const void* d_out, std::vector<uint32_t>& idx) {
    if (!c || !seed32 ||
        (n && (!d_out || !a.s1 || !a.s2 || !a.J || !a.T || !a.chal || (nresp && !a.resp) ||
               (r && (!rev_idx || !a.rev)))))
        return CC_ERR_DECODE;
    if (r && !rev_idx) return CC_ERR_DECODE;  // n = 0 with a revealed set still needs its indices
    if (cc_status s = prove_checks(c, true, q, r, nresp, rev_idx, idx)) return s;
    if (n > kMaxBatch || !cc::locate::valid_seg(seg, kMaxBatch) || cc::locate::segments(n, seg) > kMaxParts)
        return CC_ERR_DECODE;
    return CC_OK;
}

cc_status pok_partial_seg(cc_ctx* c, size_t n, size_t q, size_t r, size_t seg, uint64_t base_index,
                          const uint8_t* seed32, const PokArrays& a, const std::vector<uint32_t>& idx,
                          uint32_t* d_partials, hipStream_t st) {
    const size_t S = cc::locate::segments(n, seg);
    const size_t jtab_b = (n * 15 * 84 + 72 * 12) * 4;  // the tables of d J (cc_pok_rlc_partial_device)
    const bool twin = pok_rlc_twin(c, n);
    drain_slots(c);  // concurrent batches (cc_set_concurrency) may still use the buffers sized below
    if (cc_status s = ensure_work(c, n)) return s;
    RlcWork w = ctx_rlc_work(c);
    if (rlc_ensure(c, w, n, nullptr, jtab_b, twin) || c->seg_any.ensure((S + 1) * 4) ||
        c->seg_work.ensure(cck_fold_seg_words(c->mode, n, seg) * 4) || c->pok_idx.ensure(idx.size() * 4))
        return CC_ERR_HIP;
    StreamOrder order(c, st);
    HIPCK(hipMemcpyAsync(c->pok_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
    return launch_pok_partial_seg(c, w, n, q, r, seg, twin, base_index, seed32, a, c->pok_idx.as<uint32_t>(),
                                  d_partials, st);
}

// the drivers' device form: verdicts for proofs [0, n) with deltas i
cc_status pok_locate_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, size_t seg, const uint8_t* seed32,
                            const PokArrays& a, const uint64_t* rev_idx, const std::vector<uint32_t>& idx,
                            uint8_t* d_verdicts, uint32_t* stats3, void* stream) {
    const size_t S = cc::locate::segments(n, seg);
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (c->loc_parts.ensure(S * RLC_PART_WORDS * 4) || c->loc_accept.ensure(S)) return CC_ERR_HIP;
    if (cc_status s = pok_partial_seg(c, n, q, r, seg, 0, seed32, a, idx, c->loc_parts.as<uint32_t>(), st)) return s;
    if (cc_status s = cc_rlc_finish_each_device(c, S, c->loc_parts.as<uint32_t>(), c->loc_accept.as<uint8_t>(),
                                                nullptr, st))
        return s;
    std::vector<uint8_t> accept(S, 0);
    KCK(HipMem::d2h(accept.data(), c->loc_accept.p, S, st));
    KCK(HipMem::sync(st));  // the one synchronisation: the accept bytes decide what is launched next
    const cc::locate::Plan p = cc::locate::plan(n, seg, accept.data());
    if (stats3) stats3[0] = (uint32_t)p.segments, stats3[1] = (uint32_t)p.rejected, stats3[2] = (uint32_t)p.rechecked;
    if (p.in_place())  // nothing to skip: per proof where the batch lies
        return cc_pok_verify_batch_device(c, n, q, r, nresp, a.s1, a.s2, a.J, a.T, a.resp, a.chal, rev_idx, a.rev,
                                          d_verdicts, nullptr, st);
    HIPCK(hipMemsetAsync(d_verdicts, 1, n, st));  // every proof of an accepted segment verifies
    if (!p.rechecked) return CC_OK;
    // the rejected runs' rows side by side, ONE per-proof launch sequence over them, verdicts back
    const size_t m = p.rechecked, sb = (size_t)sig_bytes(c->mode), ob = (size_t)oth_bytes(c->mode);
    // row widths of sigma'_1, sigma'_2, J, T, responses, challenges, revealed messages
    const size_t wd[7] = {sb, sb, ob, ob, nresp * 48, 48, r * 48};
    const uint8_t* src[7] = {a.s1, a.s2, a.J, a.T, a.resp, a.chal, a.rev};
    DevBuf* dst[7] = {&c->loc_s1, &c->loc_s2, &c->loc_pok[0], &c->loc_pok[1], &c->loc_pok[2], &c->loc_pok[3],
                      &c->loc_pok[4]};
    for (int k = 0; k < 7; k++)
        if (dst[k]->ensure(m * wd[k] + 16)) return CC_ERR_HIP;
    if (c->loc_verdicts.ensure(m)) return CC_ERR_HIP;
    auto d2d = [&](void* d, const void* s, size_t bytes) {
        return bytes ? hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
    };
    for (const cc::locate::Run& run : p.runs)
        for (int k = 0; k < 7; k++)
            HIPCK(d2d(dst[k]->as<uint8_t>() + run.off * wd[k], src[k] + run.lo * wd[k], (run.hi - run.lo) * wd[k]));
    if (cc_status s = cc_pok_verify_batch_device(c, m, q, r, nresp, dst[0]->as<uint8_t>(), dst[1]->as<uint8_t>(),
                                                 dst[2]->as<uint8_t>(), dst[3]->as<uint8_t>(), dst[4]->as<uint8_t>(),
                                                 dst[5]->as<uint8_t>(), rev_idx, dst[6]->as<uint8_t>(),
                                                 c->loc_verdicts.as<uint8_t>(), nullptr, st))
        return s;
    for (const cc::locate::Run& run : p.runs)
        HIPCK(d2d(d_verdicts + run.lo, c->loc_verdicts.as<uint8_t>() + run.off, run.hi - run.lo));
    return CC_OK;
}

inline size_t pok_default_seg(int mode) {
    return mode == 0 ? CC_POK_LOCATE_SEG_DEFAULT_G2 : CC_POK_LOCATE_SEG_DEFAULT_G1;
}

}  // namespace

cc_status cc_pok_rlc_partial_seg_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, size_t seg,
                                        uint64_t base_index, const uint8_t* seed32, const uint8_t* d_s1,
                                        const uint8_t* d_s2, const uint8_t* d_J, const uint8_t* d_T,
                                        const uint8_t* d_resp, const uint8_t* d_chal, const uint64_t* rev_idx,
                                        const uint8_t* d_rev_msgs, uint32_t* d_partials, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    const PokArrays a{d_s1, d_s2, d_J, d_T, d_resp, d_chal, d_rev_msgs};
    std::vector<uint32_t> idx;
    if (cc_status s = pok_seg_checks(c, n, q, r, nresp, seg, seed32, a, rev_idx, d_partials, idx)) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    return pok_partial_seg(c, n, q, r, seg, base_index, seed32, a, idx, d_partials,
                           stream ? (hipStream_t)stream : c->stream);
}

cc_status cc_pok_verify_batch_locate_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, size_t seg,
                                            const uint8_t* seed32, const uint8_t* d_s1, const uint8_t* d_s2,
                                            const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_resp,
                                            const uint8_t* d_chal, const uint64_t* rev_idx, const uint8_t* d_rev_msgs,
                                            uint8_t* d_verdicts, uint32_t* stats3, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!seg && c) seg = pok_default_seg(c->mode);
    const PokArrays a{d_s1, d_s2, d_J, d_T, d_resp, d_chal, d_rev_msgs};
    std::vector<uint32_t> idx;
    if (cc_status s = pok_seg_checks(c, n, q, r, nresp, seg, seed32, a, rev_idx, d_verdicts, idx)) return s;
    if (stats3) stats3[0] = stats3[1] = stats3[2] = 0;
    if (!n) return CC_OK;
    return pok_locate_device(c, n, q, r, nresp, seg, seed32, a, rev_idx, idx, d_verdicts, stats3, stream);
}

cc_status cc_pok_verify_batch_locate(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, size_t seg,
                                     const uint8_t* s1, const uint8_t* s2, const uint8_t* J, const uint8_t* T,
                                     const uint8_t* resp, const uint8_t* chal, const uint64_t* rev_idx,
                                     const uint8_t* rev_msgs, uint8_t* verdicts, uint32_t* stats3) {
    c = primary(c);  // a device set forwards to its first device, as every PoK host form does
    if (!seg && c) seg = pok_default_seg(c->mode);
    uint8_t seed[32] = {0};
    std::vector<uint32_t> idx;
    const PokArrays host{s1, s2, J, T, resp, chal, rev_msgs};
    if (cc_status s = pok_seg_checks(c, n, q, r, nresp, seg, seed, host, rev_idx, verdicts, idx)) return s;
    if (stats3) stats3[0] = stats3[1] = stats3[2] = 0;
    if (!n) return CC_OK;
    if (fresh_seed(seed)) return CC_ERR_HIP;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches may still read the input buffers
    const size_t sb = (size_t)sig_bytes(c->mode), ob = (size_t)oth_bytes(c->mode);
    DevBuf &dJ = c->in_aux[0], &dT = c->in_aux[1], &dR = c->in_aux[2], &dC = c->in_aux[3], &dM = c->in_aux[4];
    if (c->in_s1.ensure(n * sb) || c->in_s2.ensure(n * sb) || dJ.ensure(n * ob) || dT.ensure(n * ob) ||
        dR.ensure(n * nresp * 48 + 16) || dC.ensure(n * 48) || dM.ensure(n * r * 48 + 16) || c->verdicts.ensure(n))
        return CC_ERR_HIP;
    HostForm f(c->stream);
    f.up(c->in_s1, s1, n * sb);
    f.up(c->in_s2, s2, n * sb);
    f.up(dJ, J, n * ob);
    f.up(dT, T, n * ob);
    f.up(dR, resp, n * nresp * 48);
    f.up(dC, chal, n * 48);
    f.up(dM, rev_msgs, n * r * 48);
    f.launch([&] {
        const PokArrays d{c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(), dJ.as<uint8_t>(), dT.as<uint8_t>(),
                          dR.as<uint8_t>(), dC.as<uint8_t>(), dM.as<uint8_t>()};
        return pok_locate_device(c, n, q, r, nresp, seg, seed, d, rev_idx, idx, c->verdicts.as<uint8_t>(), stats3,
                                 c->stream);
    });
    f.down(verdicts, c->verdicts, n);
    return f.finish();
}
