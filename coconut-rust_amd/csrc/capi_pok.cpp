// C ABI, PoKOfSignatureProof::verify: shared verkey, RLC batch mode, one verkey per proof (ctx.h).
#include "ctx.h"

// revealed indices (shared by the batch): < q and unique (ps_sig's HashMap keys); reference would panic
static cc_status check_revealed(size_t q, size_t r, const uint64_t* rev_idx, std::vector<uint32_t>& idx) {
    idx.assign(r ? r : 1, 0);
    for (size_t z = 0; z < r; z++) {
        if (rev_idx[z] >= q) return CC_ERR_LEN;  // reference would index out of bounds (panic)
        for (size_t y = 0; y < z; y++)
            if (rev_idx[y] == rev_idx[z]) return CC_ERR_DECODE;  // HashMap keys are unique
        idx[z] = (uint32_t)rev_idx[z];
    }
    return CC_OK;
}

// the checks of the PoK forms after the NULL checks, in the header's order; with_vk: verify and
// PoKOfSignature::init need the verkey's tables, gen_proof only the shape
cc_status cc::host::prove_checks(const cc_ctx* c, bool with_vk, size_t q, size_t r, size_t nresp, const uint64_t* rev_idx,
                                 std::vector<uint32_t>& idx) {
    if (with_vk) {
        if (!c->have_params || !c->have_vk) return CC_ERR_STATE;
        if (q != c->q) return CC_ERR_LEN;
    } else if (q > kMaxQ) {
        return CC_ERR_DECODE;
    }
    // more than q indices hold one >= q or a repeated one among the first q + 1
    cc_status s = check_revealed(q, std::min(r, q + 1), rev_idx, idx);
    if (s) return s;
    if (nresp != q - r + 1) return CC_ERR_BASES_EXPS;
    return CC_OK;
}

static cc_status launch_pok(cc_ctx* c, const VerifyWork& w, size_t n, size_t q, size_t r, const uint8_t* d_s1,
                            const uint8_t* d_s2, const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_resp,
                            const uint8_t* d_chal, const uint32_t* d_idx, const uint8_t* d_rev_msgs, uint8_t* d_verdicts,
                            uint8_t* d_gt, hipStream_t st) {
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
    // small batches: one block of two waves per proof (the Schnorr terms over a wave's lanes)
    KCK((n <= kPrepWideMax ? cck_prep_pok_wide : cck_prep_pok)(
        c->mode, n, (int)q, (int)r, d_s1, d_s2, d_J, d_T, d_resp, d_chal, d_rev_msgs, d_idx, c->vk_aff.as<uint32_t>(),
        c->X_inf, c->table.as<uint32_t>(), c->wbits, c->table_inf.as<uint32_t>(), w.prep->as<uint32_t>(),
        w.flags->as<uint32_t>(), w.scratch->as<uint32_t>(), st));  // J*chal window table: the fexp scratch, free until fexp
    return launch_pairings(c, w, n, d_verdicts, d_gt, st);
}

// The PoK partial's Miller launch.  The four-proof loop (k_miller4) runs one wave a SIMD and fills the
// chip only from 128 proofs a SIMD on (131,072 on 1,024 SIMDs); a batch of half that leaves every
// second SIMD idle for the whole loop.  While the two-proof loop's waves (64 proofs each) still fit one
// a SIMD it is the shorter launch: the same twin layout, twice the Miller values for the product tree.
bool cc::host::pok_rlc_twin(cc_ctx* c, size_t n) {
    if (!c->n_simd) {
        int cu = 0;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cu <= 0) {
            (void)hipGetLastError();
            cu = 256;
        }
        c->n_simd = 4 * cu;
    }
    return (n + 63) / 64 <= (size_t)c->n_simd;
}

cc_status cc_pok_verify_batch_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* d_s1,
                                     const uint8_t* d_s2, const uint8_t* d_J, const uint8_t* d_T,
                                     const uint8_t* d_resp, const uint8_t* d_chal, const uint64_t* rev_idx,
                                     const uint8_t* d_rev_msgs, uint8_t* d_verdicts, uint8_t* d_gt, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_s1 || !d_s2 || !d_J || !d_T || !d_chal || !d_verdicts || (nresp && !d_resp) ||
                     (r && (!rev_idx || !d_rev_msgs)))))
        return CC_ERR_DECODE;
    std::vector<uint32_t> idx;
    cc_status s = prove_checks(c, true, q, r, nresp, rev_idx, idx);
    if (s) return s;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (c->concurrency > 1) {  // the next concurrency slot (cc_set_concurrency): its own tables of d J
        const cc::slots::Sizes sz = cc::slots::verify_sizes(n, 0, (n * 15 * 84 + 72 * 12) * 4, idx.size() * 4 + 4);
        return on_slot(c, st, sz, [&](int k, const VerifyWork& w) -> cc_status {
            if (r) KCK(c->stage[(size_t)k].upload(c->dev, w.idx->p, idx.data(), idx.size() * 4, st));  // pinned ring
            return launch_pok(c, w, n, q, r, d_s1, d_s2, d_J, d_T, d_resp, d_chal, w.idx->as<uint32_t>(), d_rev_msgs,
                              d_verdicts, d_gt, st);
        });
    }
    s = ensure_work(c, n);
    if (s) return s;
    StreamOrder order(c, st);
    if (c->pok_idx.ensure(idx.size() * 4)) return CC_ERR_HIP;
    HIPCK(hipMemcpyAsync(c->pok_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
    s = launch_pok(c, ctx_work(c), n, q, r, d_s1, d_s2, d_J, d_T, d_resp, d_chal, c->pok_idx.as<uint32_t>(), d_rev_msgs,
                   d_verdicts, d_gt, st);
    if (s) return s;
    if (c->timing) collect_timing(c);
    return CC_OK;
}

// The PoK form of cc_rlc_partial_device (pok_rlc.hip): arguments and errors of
// cc_pok_verify_batch_device, slots and ordering of cc_rlc_partial_device.
cc_status cc_pok_rlc_partial_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, uint64_t base_index,
                                    const uint8_t* seed32, const uint8_t* d_s1, const uint8_t* d_s2,
                                    const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_resp,
                                    const uint8_t* d_chal, const uint64_t* rev_idx, const uint8_t* d_rev_msgs,
                                    uint32_t* d_partial, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !seed32 || !d_partial ||
        (n && (!d_s1 || !d_s2 || !d_J || !d_T || !d_chal || (nresp && !d_resp) || (r && (!rev_idx || !d_rev_msgs)))))
        return CC_ERR_DECODE;
    std::vector<uint32_t> idx;
    cc_status s = prove_checks(c, true, q, r, nresp, rev_idx, idx);
    if (s) return s;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (!n) return write_neutral_partial(d_partial, st);
    const size_t jtab_b = (n * 15 * 84 + 72 * 12) * 4;  // the tables of d J (ensure_work)
    PokRlcArgs pok{r, d_J, d_T, d_resp, d_chal, d_rev_msgs, nullptr, pok_rlc_twin(c, n)};
    if (c->concurrency > 1) {  // the next concurrency slot (cc_set_concurrency): its own workspaces
        const cc::slots::Sizes sz = cc::slots::verify_sizes(n, 0, jtab_b, idx.size() * 4 + 4);
        return on_slot(c, st, sz, [&](int k, const VerifyWork& w) -> cc_status {
            RlcWork rw = slot_rlc_work(c, k);
            if (rlc_ensure(c, rw, n, &c->pool.recs[(size_t)k], jtab_b, pok.twin)) return CC_ERR_HIP;
            if (r) KCK(c->stage[(size_t)k].upload(c->dev, w.idx->p, idx.data(), idx.size() * 4, st));  // pinned ring
            pok.d_idx = w.idx->as<uint32_t>();
            return launch_rlc_partial(c, rw, n, q, base_index, seed32, d_s1, d_s2, nullptr, d_partial, st,
                                      &c->stage[(size_t)k], &pok);
        });
    }
    drain_slots(c);  // concurrent batches (cc_set_concurrency) may still use the buffers sized below
    s = ensure_work(c, n);
    if (s) return s;
    RlcWork rw = ctx_rlc_work(c);
    if (rlc_ensure(c, rw, n, nullptr, jtab_b, pok.twin)) return CC_ERR_HIP;
    StreamOrder order(c, st);
    if (c->pok_idx.ensure(idx.size() * 4)) return CC_ERR_HIP;
    HIPCK(hipMemcpyAsync(c->pok_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
    pok.d_idx = c->pok_idx.as<uint32_t>();
    return launch_rlc_partial(c, rw, n, q, base_index, seed32, d_s1, d_s2, nullptr, d_partial, st, nullptr, &pok);
}

// the host forms: one upload, then (rlc) the whole-batch check first, the per-proof path on reject
static cc_status pok_host(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* s1, const uint8_t* s2,
                          const uint8_t* J, const uint8_t* T, const uint8_t* resp, const uint8_t* chal,
                          const uint64_t* rev_idx, const uint8_t* rev_msgs, uint8_t* verdicts, uint8_t* gt, int rlc) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!s1 || !s2 || !J || !T || !chal || !verdicts || (nresp && !resp) || (r && (!rev_idx || !rev_msgs)))))
        return CC_ERR_DECODE;
    std::vector<uint32_t> idx;
    cc_status s = prove_checks(c, true, q, r, nresp, rev_idx, idx);
    if (s) return s;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches still using slot 0's workspaces (cc_set_concurrency)
    size_t sb = (size_t)sig_bytes(c->mode), ob = (size_t)oth_bytes(c->mode);
    hipStream_t st = c->stream;
    DevBuf &dJ = c->in_aux[0], &dT = c->in_aux[1], &dR = c->in_aux[2], &dC = c->in_aux[3], &dM = c->in_aux[4],
           &dI = c->in_aux[5];
    if (c->in_s1.ensure(n * sb) || c->in_s2.ensure(n * sb) || dJ.ensure(n * ob) || dT.ensure(n * ob) ||
        dR.ensure(n * nresp * 48 + 16) || dC.ensure(n * 48) || dM.ensure(n * r * 48 + 16) || dI.ensure(r * 4 + 4) ||
        c->verdicts.ensure(n) || (gt && c->gt.ensure(n * 576)))
        return CC_ERR_HIP;
    s = ensure_work(c, n);
    if (s) return s;
    // the per-proof launch and its downloads: the end of h's sequence
    auto per_proof = [&](HostForm& h) -> cc_status {
        h.launch([&] {
            return launch_pok(c, ctx_work(c), n, q, r, c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(), dJ.as<uint8_t>(),
                              dT.as<uint8_t>(), dR.as<uint8_t>(), dC.as<uint8_t>(), dI.as<uint32_t>(), dM.as<uint8_t>(),
                              c->verdicts.as<uint8_t>(), gt ? c->gt.as<uint8_t>() : nullptr, st);
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
    f.up(dJ, J, n * ob);
    f.up(dT, T, n * ob);
    f.up(dR, resp, n * nresp * 48);
    f.up(dC, chal, n * 48);
    f.up(dM, rev_msgs, n * r * 48);
    f.up(dI, idx.data(), r * 4);
    if (!rlc) return per_proof(f);
    // whole-batch check; on reject (a bad proof, an identity sigma' or a J outside the subgroup somewhere) per proof
    return rlc_host(c, f, n, verdicts, [&](const uint8_t* seed) {
        return cc_pok_rlc_partial_device(c, n, q, r, nresp, 0, seed, c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(),
                                         dJ.as<uint8_t>(), dT.as<uint8_t>(), dR.as<uint8_t>(), dC.as<uint8_t>(), rev_idx,
                                         dM.as<uint8_t>(), c->rlc_part.as<uint32_t>(), st);
    }, per_proof);
}

cc_status cc_pok_verify_batch(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* s1,
                              const uint8_t* s2, const uint8_t* J, const uint8_t* T, const uint8_t* resp,
                              const uint8_t* chal, const uint64_t* rev_idx, const uint8_t* rev_msgs,
                              uint8_t* verdicts, uint8_t* gt) {
    return pok_host(c, n, q, r, nresp, s1, s2, J, T, resp, chal, rev_idx, rev_msgs, verdicts, gt, 0);
}

cc_status cc_pok_verify_batch_rlc(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* s1,
                                  const uint8_t* s2, const uint8_t* J, const uint8_t* T, const uint8_t* resp,
                                  const uint8_t* chal, const uint64_t* rev_idx, const uint8_t* rev_msgs,
                                  uint8_t* verdicts) {
    return pok_host(c, n, q, r, nresp, s1, s2, J, T, resp, chal, rev_idx, rev_msgs, verdicts, nullptr, 1);
}

// ---------------------------------------------------------------- PoK verify, one verkey per proof
// (pok_pervk.hip): the prep's Straus tables live in w.vkb, the rest is launch_pok's
static cc_status launch_pok_pervk(cc_ctx* c, const VerifyWork& w, size_t n, size_t q, size_t r, const uint8_t* d_s1,
                                  const uint8_t* d_s2, const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_resp,
                                  const uint8_t* d_chal, const uint32_t* d_idx, const uint8_t* d_rev_msgs,
                                  const uint8_t* d_vkX, const uint8_t* d_vkY, uint8_t* d_verdicts, uint8_t* d_gt,
                                  hipStream_t st) {
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
    KCK(cck_prep_pok_var(c->mode, n, (int)q, (int)r, d_s1, d_s2, d_J, d_T, d_resp, d_chal, d_rev_msgs, d_idx, d_vkX,
                         d_vkY, c->gtilde_aff.as<uint32_t>(), c->gtilde_inf, w.vkb->as<uint32_t>(),
                         w.prep->as<uint32_t>(), w.flags->as<uint32_t>(), st));
    return launch_pairings(c, w, n, d_verdicts, d_gt, st);
}

// the checks of cc_pok_verify_batch_device in its order, without a loaded verkey (q <= the pervk ceiling)
static cc_status pok_pervk_check(const cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const void* s1,
                                 const void* s2, const void* J, const void* T, const void* resp, const void* chal,
                                 const uint64_t* rev_idx, const void* rev_msgs, const void* vkX, const void* vkY,
                                 const void* verdicts, std::vector<uint32_t>& idx) {
    if (!c || (n && (!s1 || !s2 || !J || !T || !chal || !verdicts || !vkX || (q && !vkY) || (nresp && !resp) ||
                     (r && (!rev_idx || !rev_msgs)))))
        return CC_ERR_DECODE;
    if (!c->have_params) return CC_ERR_STATE;
    if (q > 4096) return CC_ERR_DECODE;
    if (r && !rev_idx) return CC_ERR_DECODE;  // n = 0 with a revealed set still needs its indices
    cc_status s = check_revealed(q, r, rev_idx, idx);
    if (s) return s;
    if (nresp != q - r + 1) return CC_ERR_BASES_EXPS;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    return CC_OK;
}

cc_status cc_pok_verify_batch_pervk_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp,
                                           const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_J,
                                           const uint8_t* d_T, const uint8_t* d_resp, const uint8_t* d_chal,
                                           const uint64_t* rev_idx, const uint8_t* d_rev_msgs, const uint8_t* d_vkX,
                                           const uint8_t* d_vkY, uint8_t* d_verdicts, uint8_t* d_gt, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    std::vector<uint32_t> idx;
    cc_status s = pok_pervk_check(c, n, q, r, nresp, d_s1, d_s2, d_J, d_T, d_resp, d_chal, rev_idx, d_rev_msgs, d_vkX,
                                  d_vkY, d_verdicts, idx);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t vkw = cck_prep_pok_var_words(c->mode, n, q) * 4;
    if (c->concurrency > 1) {  // the next concurrency slot (cc_set_concurrency): its own tables and indices
        const cc::slots::Sizes sz = cc::slots::verify_sizes(n, vkw, 0, idx.size() * 4 + 4);
        return on_slot(c, st, sz, [&](int k, const VerifyWork& w) -> cc_status {
            if (r) KCK(c->stage[(size_t)k].upload(c->dev, w.idx->p, idx.data(), idx.size() * 4, st));  // pinned ring
            return launch_pok_pervk(c, w, n, q, r, d_s1, d_s2, d_J, d_T, d_resp, d_chal, w.idx->as<uint32_t>(),
                                    d_rev_msgs, d_vkX, d_vkY, d_verdicts, d_gt, st);
        });
    }
    s = ensure_work(c, n);
    if (s) return s;
    if (c->vkb.bytes < vkw) drain_slots(c);  // slot 0's batch may still read it
    StreamOrder order(c, st);
    if (c->vkb.ensure(vkw) || c->pok_idx.ensure(idx.size() * 4)) return CC_ERR_HIP;
    HIPCK(hipMemcpyAsync(c->pok_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
    s = launch_pok_pervk(c, ctx_work(c), n, q, r, d_s1, d_s2, d_J, d_T, d_resp, d_chal, c->pok_idx.as<uint32_t>(),
                         d_rev_msgs, d_vkX, d_vkY, d_verdicts, d_gt, st);
    if (s) return s;
    if (c->timing) collect_timing(c);
    return CC_OK;
}

// the host form: one upload, the device form on the context's stream, one download
cc_status cc_pok_verify_batch_pervk(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* s1,
                                    const uint8_t* s2, const uint8_t* J, const uint8_t* T, const uint8_t* resp,
                                    const uint8_t* chal, const uint64_t* rev_idx, const uint8_t* rev_msgs,
                                    const uint8_t* vkX, const uint8_t* vkY, uint8_t* verdicts, uint8_t* gt) {
    c = primary(c);  // a device set forwards to its first device
    std::vector<uint32_t> idx;
    cc_status s = pok_pervk_check(c, n, q, r, nresp, s1, s2, J, T, resp, chal, rev_idx, rev_msgs, vkX, vkY, verdicts, idx);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches may still read the staging buffers
    const size_t sb = (size_t)sig_bytes(c->mode), ob = (size_t)oth_bytes(c->mode);
    hipStream_t st = c->stream;
    DevBuf &dJ = c->in_aux[0], &dT = c->in_aux[1], &dR = c->in_aux[2], &dC = c->in_aux[3], &dM = c->in_aux[4];
    if (c->in_s1.ensure(n * sb) || c->in_s2.ensure(n * sb) || dJ.ensure(n * ob) || dT.ensure(n * ob) ||
        dR.ensure(n * nresp * 48 + 16) || dC.ensure(n * 48) || dM.ensure(n * r * 48 + 16) || c->in_vkX.ensure(n * ob) ||
        c->in_vkY.ensure(n * q * ob + 16) || c->verdicts.ensure(n) || (gt && c->gt.ensure(n * 576)))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up(c->in_s1, s1, n * sb);
    f.up(c->in_s2, s2, n * sb);
    f.up(dJ, J, n * ob);
    f.up(dT, T, n * ob);
    f.up(dR, resp, n * nresp * 48);
    f.up(dC, chal, n * 48);
    f.up(dM, rev_msgs, n * r * 48);
    f.up(c->in_vkX, vkX, n * ob);
    f.up(c->in_vkY, vkY, n * q * ob);
    f.launch([&] {
        return cc_pok_verify_batch_pervk_device(c, n, q, r, nresp, c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(),
                                                dJ.as<uint8_t>(), dT.as<uint8_t>(), dR.as<uint8_t>(), dC.as<uint8_t>(),
                                                rev_idx, dM.as<uint8_t>(), c->in_vkX.as<uint8_t>(),
                                                c->in_vkY.as<uint8_t>(), c->verdicts.as<uint8_t>(),
                                                gt ? c->gt.as<uint8_t>() : nullptr, st);
    });
    f.down(verdicts, c->verdicts, n);
    f.down(gt, c->gt, gt ? n * 576 : 0);
    return f.finish();
}
