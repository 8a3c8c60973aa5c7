// C ABI, Signature::verify: the verify launches, the device and host forms, the RLC partial and finish, and
// the sharded verify of a device set (ctx.h).  The segmented partial, the per-partial finish and the locate
// drivers: capi_locate.cpp.
#include "ctx.h"

// Small batches run latency-bound: their Miller loops one wave per pair (n <= kWideMax: miller_wide.hip
// k_wide_pairs -> k_miller_wide -> fexp_pl.hip k_f12_reduce_wide) instead of one lane pair per credential (k_miller:
// one 2-pair loop's latency on a lone wave, ~7.5 ms for any batch up to a few thousand), and their
// final exponentiation one wave per credential (n <= kFexpWideMax: k_fexp1, 1.33 ms) instead of a lane
// quad (k_fexp_q: ~3 ms floor).  Both wide kernels hold one wave a SIMD: 1,024 waves a round of the
// chip, i.e. 512 credentials a round of the Miller path (0.8 ms a round: eight rounds at 4,096, 6.4 ms,
// under the pair-lane loop's ~7.5-9 ms latency there), 1,024 of the fexp (two rounds, ~2.7 ms, still
// under the quad kernel's floor at 2,048).  The shared-verkey prep takes its one-wave form up to
// kFexpWideMax, the PoK and per-credential-verkey preps up to kPrepWideMax.  Measured:
// profiles/r05/wide_spread, thresholds, miller_wide_pipe, fexp_thr.
// (the thresholds live in slots.h with the workspace sizes they decide; k_miller_wide2, two waves a
// pair, takes launches of <= kWide2Max = 256 pairs, i.e. <= 128 credentials: miller_wide.hip)

// the three verify launches on device buffers (VerifyWork, slots.h); timing per phase when enabled.
// d_vkX == NULL: the shared verkey's tables; else one verkey per credential (d_vkX n x OtherGroup, d_vkY
// n x q x OtherGroup; the Straus MSM of pervk.hip, its scratch in w.vkb, sized by the caller)
// the batch's Miller values into w.fbuf (SoA stride n): n <= kWideMax one wave per pair, else the
// pair-lane loop (one lane pair per credential, both pairs with a shared squaring)
static cc_status launch_miller(cc_ctx* c, const VerifyWork& w, size_t n, hipStream_t st) {
    if (n <= kWideMax) {
        const size_t m = 2 * n;
        KCK(cck_wide_pairs(c->mode, n, n, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(), c->gtilde_aff.as<uint32_t>(),
                           w.wprep->as<uint32_t>(), w.wflags->as<uint32_t>(), st));
        KCK(cck_miller_wide(m, w.wprep->as<uint32_t>(), w.wflags->as<uint32_t>(), w.wf->as<uint32_t>(), m, 0, st));
        KCK(cck_f12_reduce_wide(m, w.wf->as<uint32_t>(), w.fbuf->as<uint32_t>(), st));
        return CC_OK;
    }
    // one credential per lane pair (tower_pl.h), Miller values to SoA elements [0, n) of stride n; the constant:
    // SigG2 g~ affine G1 in the lazy R' form (24 words), SigG1 g~'s Miller lines (68 x 72 words)
    KCK(c->mode == 0 ? cck_miller_lz_g2(0, n, n, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                        c->gtilde_lz.as<uint32_t>(), w.fbuf->as<uint32_t>(), n, 0, nullptr, st)
                     : cck_miller_lz_g1(0, n, n, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                        c->gtilde_lines.as<uint32_t>(), w.fbuf->as<uint32_t>(), n, 0, nullptr, st));
    return CC_OK;
}
// after a prep (phase 0 of the timing): the Miller loops and the final exponentiation of the n values
cc_status cc::host::launch_pairings(cc_ctx* c, const VerifyWork& w, size_t n, uint8_t* d_verdicts, uint8_t* d_gt,
                                    hipStream_t st) {
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    // a g~ that did not decode is the identity: pair 1 is skipped (factor 1), as the reference pairs it
    if (c->gtilde_inf) KCK(cck_flag_pair1(n, w.flags->as<uint32_t>(), st));
    cc_status ms = launch_miller(c, w, n, st);
    if (ms) return ms;
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    // n <= kFexpWideMax: one wave per credential (k_fexp1, its chain in w.scratch: 72 x 12 x n words)
    KCK(cck_fexp(n, w.fbuf->as<uint32_t>(), w.scratch->as<uint32_t>(), w.flags->as<uint32_t>(), d_verdicts, d_gt,
                 kFexpWideMax, st));
    if (c->timing) (void)hipEventRecord(c->ev[3], st);
    return CC_OK;
}
static cc_status launch_verify(cc_ctx* c, const VerifyWork& w, size_t n, size_t q, const uint8_t* d_s1,
                               const uint8_t* d_s2, const uint8_t* d_msgs, const uint8_t* d_vkX, const uint8_t* d_vkY,
                               uint8_t* d_verdicts, uint8_t* d_gt, hipStream_t st) {
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
    if (d_vkX)
        KCK(cck_prep_var(c->mode, n, (int)q, d_s1, d_s2, d_vkX, d_vkY, d_msgs, w.vkb->as<uint32_t>(),
                         w.prep->as<uint32_t>(), w.flags->as<uint32_t>(), n <= kPrepWideMax, st));
    else  // small batches: one wave per credential, the MSM's window terms over its lanes
        KCK((n <= kFexpWideMax ? cck_prep_wide : cck_prep)(c->mode, n, (int)q, d_s1, d_s2, d_msgs,
                                                       c->vk_aff.as<uint32_t>(), c->X_inf, c->table.as<uint32_t>(),
                                                       c->wbits, c->table_inf.as<uint32_t>(), w.prep->as<uint32_t>(),
                                                       w.flags->as<uint32_t>(), st));
    return launch_pairings(c, w, n, d_verdicts, d_gt, st);
}

// the *_device verify calls: with one slot, ordered against everything on the context (StreamOrder);
// with K > 1 (cc_set_concurrency), on the next slot round-robin, ordered only after the context
// stream's queued work (tables, params) and that slot's previous batch.
static cc_status verify_device(cc_ctx* c, size_t n, size_t q, const uint8_t* d_s1, const uint8_t* d_s2,
                               const uint8_t* d_msgs, const uint8_t* d_vkX, const uint8_t* d_vkY, uint8_t* d_verdicts,
                               uint8_t* d_gt, void* stream) {
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t vkw = d_vkX ? cck_prep_var_words(c->mode, n, q) * 4 : 0;
    cc_status s;
    if (c->concurrency <= 1) {
        s = ensure_work(c, n);
        if (s) return s;
        if (d_vkX && c->vkb.bytes < vkw) drain_slots(c);  // slot 0's batch may still read it
        StreamOrder order(c, st);
        if (d_vkX && c->vkb.ensure(vkw)) return CC_ERR_HIP;
        s = launch_verify(c, ctx_work(c), n, q, d_s1, d_s2, d_msgs, d_vkX, d_vkY, d_verdicts, d_gt, st);
    } else {
        // the slot sizes its own workspaces (slot 0's too): no ensure_work, which would grow slot 0 for a
        // batch landing on another slot and drain every slot in flight
        s = on_slot(c, st, cc::slots::verify_sizes(n, vkw, 0, 0), [&](int, const VerifyWork& w) {
            return launch_verify(c, w, n, q, d_s1, d_s2, d_msgs, d_vkX, d_vkY, d_verdicts, d_gt, st);
        });
    }
    if (!s && c->timing) collect_timing(c);
    return s;
}

// ---------------------------------------------------------------- RLC batch mode (rlc.hip)
int cc::host::fresh_seed(uint8_t seed[32]) {
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f) return -1;
    size_t got = fread(seed, 1, 32, f);
    fclose(f);
    return got == 32 ? 0 : -1;
}

// the context's own RLC workspaces (ctx.h RlcWork)
RlcWork cc::host::ctx_rlc_work(cc_ctx* c) {
    return {&c->prep, &c->flags, &c->fbuf, &c->scratch, &c->rlc_key, &c->rlc_any, &c->rlc_pts, &c->rlc_dig, &c->rlc_work};
}
// concurrency slot k's: slot 0 is the context's own
RlcWork cc::host::slot_rlc_work(cc_ctx* c, int k) {
    if (!k) return ctx_rlc_work(c);
    VerifySlot* sl = c->vslots[(size_t)k - 1];
    return {&sl->prep, &sl->flags, &sl->fbuf, &sl->scratch, &sl->rkey, &sl->rany, &sl->rpts, &sl->rdig, &sl->rwork};
}
// sizes for n credentials; a concurrency slot whose buffers must grow waits for its last batch first
// (scr_min: the PoK partial's tables of d J, which share the scratch with the product tree)
// twin: the two-proof Miller loop's (n + 1) / 2 Miller values instead of the four-proof loop's
int cc::host::rlc_ensure(cc_ctx* c, const RlcWork& r, size_t n, SlotPool::Rec* sl, size_t scr_min, bool twin) {
    const size_t PS = (n + 1) / 2, N = twin ? PS : (n + 3) / 4;
    const size_t prep_b = (size_t)PREP_SLOTS * 12 * 4 * std::max(PS, n), flags_b = n * 4, fbuf_b = N * 144 * 4,
                 scr_b = std::max(((N + 1) / 2) * 144 * 4 + n * 12 * 4 * 72, scr_min), pts_b = n * 48 * 4, dig_b = 16 * n,
                 work_b = cck_fold_words(c->mode, n) * 4;
    const bool grow = r.prep->bytes < prep_b || r.flags->bytes < flags_b || r.fbuf->bytes < fbuf_b ||
                      r.scratch->bytes < scr_b || r.key->bytes < 32 || r.any->bytes < 4 || r.pts->bytes < pts_b ||
                      r.dig->bytes < dig_b || r.work->bytes < work_b;
    if (!grow) return 0;
    if (sl && sl->recorded && hipEventSynchronize(sl->done) != hipSuccess) return -1;
    return r.prep->ensure(prep_b) || r.flags->ensure(flags_b) || r.fbuf->ensure(fbuf_b) || r.scratch->ensure(scr_b) ||
           r.key->ensure(32) || r.any->ensure(4) || r.pts->ensure(pts_b) || r.dig->ensure(dig_b) ||
           r.work->ensure(work_b);
}

cc_status cc::host::launch_rlc_partial(cc_ctx* c, const RlcWork& w, size_t n, size_t q, uint64_t base_index,
                                       const uint8_t* seed32, const uint8_t* d_s1, const uint8_t* d_s2,
                                       const uint8_t* d_msgs, uint32_t* d_partial, hipStream_t st, Staging* stage,
                                       const PokRlcArgs* pok) {
    const size_t PS = (n + 1) / 2;  // prep SoA stride (the twin layout: credentials 2 t, 2 t + 1 at element t)
    const bool twin = pok && pok->twin;
    const size_t N = twin ? PS : (n + 3) / 4;  // Miller values (four credentials' pairs each, k_miller4)
    if (stage) {  // a concurrency slot: through its pinned ring, so the host does not wait for the stream
        KCK(stage->upload(c->dev, w.key->p, seed32, 32, st));
    } else {  // pageable source: the copy is staged before the call returns
        KCK(HipMem::h2d(w.key->p, seed32, 32, st));
    }
    HIPCK(hipMemsetAsync(w.any->p, 0, 4, st));
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
    auto prep_part = [&](int part) {
        return cck_prep_rlc(c->mode, part, n, PS, (int)q, base_index, w.key->as<uint32_t>(), d_s1, d_s2, d_msgs,
                            c->table.as<uint32_t>(), c->wbits, c->table_inf.as<uint32_t>(), w.prep->as<uint32_t>(),
                            w.flags->as<uint32_t>(), w.any->as<uint32_t>(), w.pts->as<uint32_t>(),
                            w.dig->as<int8_t>(), st);
    };
    KCK(prep_part(0));  // decode, subgroup checks, the fold's inputs
    if (!c->vk_subgroup) {
        // a verkey / g~ point outside the subgroup: the linear-combination argument does not hold,
        // so the batch is never accepted here and the caller verifies per credential (exact)
        static const uint32_t one = 1;
        HIPCK(hipMemcpyAsync(w.any->p, &one, 4, hipMemcpyHostToDevice, st));
    }
    // The second pairs fold into 16 window sums S_w (fold.hip).  The fold's short kernels run alone
    // (behind a full launch each would wait milliseconds for a free slot); the window sums (16 waves)
    // then run on the high-priority side stream beside the delta MSM and land in the partial's window
    // section; their pairs e(S_w, P_w) are evaluated in the finish, once per batch over every shard
    // (rlc_part.h), so the credentials' two-per-loop Miller launch stays at (n + 1) / 2 loops (2,048
    // waves at 131,072 credentials: the chip's wave slots).
    KCK(cck_fold(c->mode, n, w.dig->as<int8_t>(), w.pts->as<uint32_t>(), w.work->as<uint32_t>(), st));
    hipStream_t side = c->side ? c->side : st;
    if (side != st) {
        HIPCK(hipEventRecord(c->ev_fork, st));
        HIPCK(hipStreamWaitEvent(side, c->ev_fork, 0));
    }
    KCK(cck_fold_window(c->mode, n, w.work->as<uint32_t>(), d_partial, side));
    if (pok)  // Schnorr check, J's subgroup test, delta X~ + sum_revealed (delta m_i) Y~_i + delta J
        KCK(cck_prep_pok_rlc(c->mode, n, PS, (int)q, (int)pok->r, base_index, w.key->as<uint32_t>(), pok->d_J, pok->d_T,
                             pok->d_resp, pok->d_chal, pok->d_rev_msgs, pok->d_idx, c->table.as<uint32_t>(), c->wbits,
                             c->table_inf.as<uint32_t>(), w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                             w.any->as<uint32_t>(), w.scratch->as<uint32_t>(), st));
    else
        KCK(prep_part(1));  // delta X~ + sum (delta m_j) Y~_j
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    // SigG2: sigma_1's subgroup test comes from this loop's T (a failure raises rlc_any: fallback)
    bool joined = false;
    if (twin && side != st) {
        // one wave a SIMD holds only if every CU is free when the loop's blocks are placed: the window
        // sums' 16 waves, where they outlast the prep (SigG1), pushed blocks onto occupied CUs, and the
        // launch then took the two-wave time (12.3 ms against 8.1).  Join the side stream first.
        HIPCK(hipEventRecord(c->ev_join, side));
        HIPCK(hipStreamWaitEvent(st, c->ev_join, 0));
        joined = true;
    }
    if (twin)  // two proofs per loop (k_miller<SIG, true>; the constant operand is unused)
        KCK(c->mode == 0 ? cck_miller_lz_g2(1, n, PS, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                            c->gtilde_lz.as<uint32_t>(), w.fbuf->as<uint32_t>(), N, 0,
                                            w.any->as<uint32_t>(), st)
                         : cck_miller_lz_g1(1, n, PS, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                            c->gtilde_lines.as<uint32_t>(), w.fbuf->as<uint32_t>(), N, 0, nullptr, st));
    else  // the credentials (pair 0 only: their second pairs are folded, fold.hip) four per lane pair through the
          // shared-squaring loop (k_miller4, 1 wave/SIMD): ceil(n / 4) Miller values, each the product of four
          // pairs' (the RLC multiplies them all), over the twin layout (prep stride PS >= ceil(n / 2))
        KCK(c->mode == 0 ? cck_miller4_lz_g2(n, PS, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                             w.fbuf->as<uint32_t>(), N, 0, w.any->as<uint32_t>(), st)
                         : cck_miller4_lz_g1(n, PS, w.prep->as<uint32_t>(), w.flags->as<uint32_t>(),
                                             w.fbuf->as<uint32_t>(), N, 0, nullptr, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    KCK(cck_rlc_reduce(N, w.fbuf->as<uint32_t>(), w.scratch->as<uint32_t>(), w.any->as<uint32_t>(), d_partial,
                       st));
    if (side != st && !joined) {  // the window section is part of the partial: the call ends when both are written
        HIPCK(hipEventRecord(c->ev_join, side));
        HIPCK(hipStreamWaitEvent(st, c->ev_join, 0));
    }
    if (c->timing) {
        (void)hipEventRecord(c->ev[3], st);
        collect_timing(c);
    }
    return CC_OK;
}

// an empty shard (a batch smaller than the rank count): the neutral partial — Fp12 one (Montgomery one
// in slot 0, zeros elsewhere), a clear fall-back flag and 16 identity window sums — so every rank still
// joins the all-gather and the product over ranks is unchanged
cc_status cc::host::write_neutral_partial(uint32_t* d_partial, hipStream_t st) {
    static const uint32_t kOne[12] = {0x03a9fb84u, 0xc57400d2u, 0x629c4a23u, 0x6147acdeu, 0x7e6d26cbu, 0x6b0f4b0bu,
                                      0xc2b7d6e1u, 0x91ecbde7u, 0x4fdd80b8u, 0xd56a23c3u, 0xf3a0d636u, 0x13317c30u};
    static const std::vector<uint32_t> kNeutral = [] {
        std::vector<uint32_t> v(RLC_PART_WORDS, 0u);
        memcpy(v.data(), kOne, sizeof(kOne));
        for (int w = 0; w < RLC_WINDOWS; w++) v[RLC_WIN_OFF + RLC_WIN_WORDS * w + 48] = 1u;
        return v;
    }();
    HIPCK(hipMemcpyAsync(d_partial, kNeutral.data(), RLC_PART_WORDS * 4, hipMemcpyHostToDevice, st));
    return CC_OK;
}

// Shard by credential over the device set.  Per-credential mode: every device verifies its slice, no
// collective.  RLC mode (shared verkey): every device reduces its slice to one RLC_PART_WORDS-word partial, ONE
// ncclAllGather over xGMI exchanges them, every device multiplies the gathered partials and runs the
// single final exponentiation; on reject every device falls back to per-credential verification.  The
// slices' staging is queued raw: it runs on several streams from several threads, which HostForm is not for.
static cc_status multi_verify(cc_ctx* c, size_t n, size_t q, const uint8_t* s1, const uint8_t* s2,
                              const uint8_t* msgs, const uint8_t* vkX, const uint8_t* vkY, uint8_t* verdicts,
                              uint8_t* gt, int rlc) {
    const size_t sb = (size_t)sig_bytes(c->mode), ob = (size_t)oth_bytes(c->mode);
    const size_t k = c->peers.size();
    if (rlc && !vkX && !gt) {
        uint8_t seed[32];
        if (fresh_seed(seed)) return CC_ERR_HIP;
        // stage each slice and compute its partial
        cc_status s = for_shards(c, n, [&](size_t d, size_t lo, size_t hi) -> cc_status {
            cc_ctx* p = c->peers[d];
            const size_t m = hi - lo;
            HIPCK(hipSetDevice(p->device));
            if (p->in_s1.ensure(m * sb + 16) || p->in_s2.ensure(m * sb + 16) || p->in_msgs.ensure(m * q * 48 + 16) ||
                p->rlc_part.ensure(RLC_PART_WORDS * 4) || p->rlc_gath.ensure(k * RLC_PART_WORDS * 4) || p->rlc_accept.ensure(1))
                return CC_ERR_HIP;
            if (m) {
                HIPCK(hipMemcpyAsync(p->in_s1.p, s1 + lo * sb, m * sb, hipMemcpyHostToDevice, p->stream));
                HIPCK(hipMemcpyAsync(p->in_s2.p, s2 + lo * sb, m * sb, hipMemcpyHostToDevice, p->stream));
                if (q) HIPCK(hipMemcpyAsync(p->in_msgs.p, msgs + lo * q * 48, m * q * 48, hipMemcpyHostToDevice, p->stream));
            }
            return cc_rlc_partial_device(p, m, q, lo, seed, p->in_s1.as<uint8_t>(), p->in_s2.as<uint8_t>(),
                                         p->in_msgs.as<uint8_t>(), p->rlc_part.as<uint32_t>(), p->stream);
        });
        if (s) return s;
        // the one exchange step: all-gather of the 3,716-byte (RLC_PART_WORDS = 929 words) partials
        if (ncclGroupStart() != ncclSuccess) return CC_ERR_RCCL;
        for (size_t d = 0; d < k; d++) {
            cc_ctx* p = c->peers[d];
            if (ncclAllGather(p->rlc_part.p, p->rlc_gath.p, RLC_PART_WORDS, ncclUint32, c->comms[d], p->stream) != ncclSuccess) {
                ncclGroupEnd();
                return CC_ERR_RCCL;
            }
        }
        if (ncclGroupEnd() != ncclSuccess) return CC_ERR_RCCL;
        std::vector<uint8_t> acc(k, 0);
        s = for_shards(c, n, [&](size_t d, size_t, size_t) -> cc_status {
            cc_ctx* p = c->peers[d];
            HIPCK(hipSetDevice(p->device));
            cc_status r = cc_rlc_finish_device(p, k, p->rlc_gath.as<uint32_t>(), p->rlc_accept.as<uint8_t>(), nullptr,
                                               p->stream);
            if (r) return r;
            HIPCK(hipMemcpyAsync(&acc[d], p->rlc_accept.p, 1, hipMemcpyDeviceToHost, p->stream));
            HIPCK(hipStreamSynchronize(p->stream));
            return CC_OK;
        });
        if (s) return s;
        for (size_t d = 1; d < k; d++)
            if (acc[d] != acc[0]) return CC_ERR_RCCL;  // every device multiplies the same gathered partials
        if (acc[0]) {
            memset(verdicts, 1, n);
            return CC_OK;
        }
    }
    // per-credential verification of every slice (also the RLC fallback)
    return for_shards(c, n, [&](size_t d, size_t lo, size_t hi) -> cc_status {
        if (hi == lo) return CC_OK;
        return cc_verify_batch(c->peers[d], hi - lo, q, s1 + lo * sb, s2 + lo * sb, msgs + lo * q * 48,
                               vkX ? vkX + lo * ob : nullptr, vkX ? vkY + lo * q * ob : nullptr, verdicts + lo,
                               gt ? gt + lo * 576 : nullptr, 0);
    });
}

cc_status cc_verify_batch_device(cc_ctx* c, size_t n, size_t q, const uint8_t* d_s1, const uint8_t* d_s2,
                                 const uint8_t* d_msgs, uint8_t* d_verdicts, uint8_t* d_gt, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_s1 || !d_s2 || !d_verdicts))) return CC_ERR_DECODE;
    if (!c->have_params || !c->have_vk) return CC_ERR_STATE;
    if (q != c->q) return CC_ERR_LEN;
    return verify_device(c, n, q, d_s1, d_s2, d_msgs, nullptr, nullptr, d_verdicts, d_gt, stream);
}

cc_status cc_verify_batch_pervk_device(cc_ctx* c, size_t n, size_t q, const uint8_t* d_s1, const uint8_t* d_s2,
                                       const uint8_t* d_msgs, const uint8_t* d_vkX, const uint8_t* d_vkY,
                                       uint8_t* d_verdicts, uint8_t* d_gt, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || q > 4096 || (n && (!d_s1 || !d_s2 || !d_vkX || !d_verdicts || (q && (!d_msgs || !d_vkY)))))
        return CC_ERR_DECODE;
    if (!c->have_params) return CC_ERR_STATE;
    return verify_device(c, n, q, d_s1, d_s2, d_msgs, d_vkX, d_vkY, d_verdicts, d_gt, stream);
}

cc_status cc_rlc_partial_device(cc_ctx* c, size_t n, size_t q, uint64_t base_index, const uint8_t* seed32,
                                const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs, uint32_t* d_partial,
                                void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !seed32 || !d_partial || (n && (!d_s1 || !d_s2 || (q && !d_msgs)))) return CC_ERR_DECODE;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!c->have_params || !c->have_vk) return CC_ERR_STATE;
    if (q != c->q) return CC_ERR_LEN;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (!n) return write_neutral_partial(d_partial, st);
    if (c->concurrency > 1) {  // the next concurrency slot (cc_set_concurrency): its own workspaces
        return on_slot(c, st, cc::slots::verify_sizes(n, 0, 0, 0), [&](int k, const VerifyWork&) -> cc_status {
            RlcWork r = slot_rlc_work(c, k);
            if (rlc_ensure(c, r, n, &c->pool.recs[(size_t)k])) return CC_ERR_HIP;
            return launch_rlc_partial(c, r, n, q, base_index, seed32, d_s1, d_s2, d_msgs, d_partial, st,
                                      &c->stage[(size_t)k]);
        });
    }
    drain_slots(c);  // concurrent batches (cc_set_concurrency) may still use the buffers sized below
    cc_status s = ensure_work(c, n);
    if (s) return s;
    RlcWork r = ctx_rlc_work(c);
    if (rlc_ensure(c, r, n, nullptr)) return CC_ERR_HIP;
    StreamOrder order(c, st);
    return launch_rlc_partial(c, r, n, q, base_index, seed32, d_s1, d_s2, d_msgs, d_partial, st, nullptr);
}

cc_status cc_rlc_finish_device(cc_ctx* c, size_t nparts, const uint32_t* d_partials, uint8_t* d_accept,
                               uint8_t* d_gt, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !nparts || nparts > kMaxParts || !d_partials || !d_accept) return CC_ERR_DECODE;
    if (!c->have_params || !c->have_vk) return CC_ERR_STATE;  // the window pairs' P_w come with the verkey
    HIPCK(hipSetDevice(c->device));
    // the finish owns its buffers (Fp12 values, window-pair operands, fexp scratch, flag) and reads only
    // the verkey's P_w, so it is NOT ordered against the context's stream: on a caller stream it may
    // overlap the next batch's cc_rlc_partial_device (the caller orders d_partials itself).  Finishes of
    // one context are ordered among themselves (ev_fin): two finishes on different streams never share
    // the buffers at the same time, whichever engines or streams issue them; a verkey change waits for
    // the last finish before it rewrites P_w.
    const size_t k = nparts, NW = (size_t)RLC_WINDOWS * k, NF = k + NW;
    if (c->rlc_flag.ensure(4) || c->fin_f.ensure(NF * 144 * 4) ||
        c->fin_scratch.ensure(std::max(((NF + 1) / 2) * 144 * 4, (size_t)2 * 72 * 12 * 4)) ||
        c->fin_prep.ensure((size_t)PREP_SLOTS * 12 * NW * 4) || c->fin_flags2.ensure(NW * 4) ||
        c->fin_part.ensure(RLC_PART_WORDS * 4))
        return CC_ERR_HIP;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (c->fin_recorded) HIPCK(hipStreamWaitEvent(st, c->ev_fin, 0));
    // the partials' products (elements 0 .. k-1) and every shard's 16 window pairs e(S_w, P_w), one wave
    // each (latency-bound: one loop's length for any k up to 16 GPUs), to elements k .. 17 k - 1; the
    // product tree multiplies all 17 k; one final exponentiation, whose flag (a sigma was the identity or
    // outside the subgroup somewhere) forces a reject
    KCK(cck_rlc_gather(c->mode, k, d_partials, c->rlc_pw.as<uint32_t>(), c->rlc_finf.as<uint8_t>(),
                       c->fin_f.as<uint32_t>(), NF, c->fin_prep.as<uint32_t>(), c->fin_flags2.as<uint32_t>(),
                       c->rlc_flag.as<uint32_t>(), st));
    KCK(cck_miller_wide(NW, c->fin_prep.as<uint32_t>(), c->fin_flags2.as<uint32_t>(), c->fin_f.as<uint32_t>(), NF, k,
                        st));
    KCK(cck_rlc_reduce(NF, c->fin_f.as<uint32_t>(), c->fin_scratch.as<uint32_t>(), c->rlc_flag.as<uint32_t>(),
                       c->fin_part.as<uint32_t>(), st));
    KCK(cck_fexp(1, c->fin_part.as<uint32_t>(), c->fin_scratch.as<uint32_t>(), c->fin_part.as<uint32_t>() + RLC_FLAG,
                 d_accept, d_gt, 1, st));
    HIPCK(hipEventRecord(c->ev_fin, st));
    c->fin_recorded = true;
    return CC_OK;
}

cc_status cc_verify_batch(cc_ctx* c, size_t n, size_t q, const uint8_t* s1, const uint8_t* s2, const uint8_t* msgs,
                          const uint8_t* vkX, const uint8_t* vkY, uint8_t* verdicts, uint8_t* gt, int rlc) {
    if (!c || (n && (!s1 || !s2 || !verdicts || (q && !msgs)))) return CC_ERR_DECODE;
    if (!c->have_params) return CC_ERR_STATE;
    const bool per_vk = vkX != nullptr;
    if (per_vk && ((q && !vkY) || q > 4096)) return CC_ERR_DECODE;
    if (!per_vk) {
        if (!c->have_vk) return CC_ERR_STATE;
        if (q != c->q) return CC_ERR_LEN;
    }
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    if (!c->peers.empty()) return multi_verify(c, n, q, s1, s2, msgs, vkX, vkY, verdicts, gt, rlc);
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches still using slot 0's workspaces (cc_set_concurrency)
    size_t sb = (size_t)sig_bytes(c->mode), ob = (size_t)oth_bytes(c->mode);
    if (c->in_s1.ensure(n * sb) || c->in_s2.ensure(n * sb) || c->in_msgs.ensure(n * q * 48 + 16) ||
        c->verdicts.ensure(n) || (gt && c->gt.ensure(n * 576)))
        return CC_ERR_HIP;
    cc_status s = ensure_work(c, n);
    if (s) return s;
    hipStream_t st = c->stream;
    // the per-credential launch and its downloads: the end of h's sequence
    auto per_credential = [&](HostForm& h) -> cc_status {
        h.launch([&] {
            return launch_verify(c, ctx_work(c), n, q, c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(),
                                 c->in_msgs.as<uint8_t>(), per_vk ? c->in_vkX.as<uint8_t>() : nullptr,
                                 per_vk ? c->in_vkY.as<uint8_t>() : nullptr, c->verdicts.as<uint8_t>(),
                                 gt ? c->gt.as<uint8_t>() : nullptr, st);
        });
        h.down(verdicts, c->verdicts, n);
        h.down(gt, c->gt, gt ? n * 576 : 0);
        const cc_status e = h.finish();
        if (!e) collect_timing(c);
        return e;
    };
    HostForm f(st);
    f.up(c->in_s1, s1, n * sb);
    f.up(c->in_s2, s2, n * sb);
    f.up(c->in_msgs, msgs, n * q * 48);
    if (rlc && !per_vk && !gt)  // whole-batch check; on reject (a bad or identity credential somewhere) per credential
        return rlc_host(c, f, n, verdicts, [&](const uint8_t* seed) {
            return cc_rlc_partial_device(c, n, q, 0, seed, c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(),
                                         c->in_msgs.as<uint8_t>(), c->rlc_part.as<uint32_t>(), st);
        }, per_credential);
    if (per_vk) {
        if (c->in_vkX.ensure(n * ob) || c->in_vkY.ensure(n * q * ob + 16) ||
            c->vkb.ensure(cck_prep_var_words(c->mode, n, q) * 4))
            return CC_ERR_HIP;
        f.up(c->in_vkX, vkX, n * ob);
        f.up(c->in_vkY, vkY, n * q * ob);
    }
    return per_credential(f);
}
