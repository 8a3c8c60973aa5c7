// C ABI, holder side: PoKOfSignature proving, BlindSignature::unblind, the request params and
// SignatureRequest / SignatureRequestPoK (ctx.h).
#include "ctx.h"

// the request forms' checks after the NULL checks, in the header's order; with_params: new and init read the tables
cc_status cc::host::rq_checks(const cc_ctx* c, bool with_params, size_t n, size_t q, size_t k) {
    if (with_params) {
        if (!c->have_rq) return CC_ERR_STATE;
        if (q != c->rq_q) return CC_ERR_LEN;
    } else if (q > kMaxQ) {
        return CC_ERR_DECODE;
    }
    if (k > q) return CC_ERR_LEN;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    return CC_OK;
}

// ---------------------------------------------------------------- holder side (pok_prove.hip)
static cc_status launch_pok_init(cc_ctx* c, size_t n, size_t q, size_t r, const uint8_t* d_s1, const uint8_t* d_s2,
                                 const uint8_t* d_msgs, const uint32_t* d_idx, const uint8_t* d_rand, uint8_t* d_o1,
                                 uint8_t* d_o2, uint8_t* d_J, uint8_t* d_T, hipStream_t st) {
    KCK(cck_sigma_prime(c->mode, n, q - r + 3, d_s1, d_s2, d_rand, c->prove_scratch.as<uint32_t>(), d_o1, d_o2, st));
    KCK(cck_pok_commit(c->mode, n, (int)q, (int)r, d_msgs, d_rand, d_idx, c->table.as<uint32_t>(), c->wbits,
                       c->table_inf.as<uint32_t>(), d_J, d_T, st));
    return CC_OK;
}

cc_status cc_pok_init_batch_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* d_s1,
                                   const uint8_t* d_s2, const uint8_t* d_msgs, const uint64_t* rev_idx,
                                   const uint8_t* d_rand, uint8_t* d_o1, uint8_t* d_o2, uint8_t* d_J, uint8_t* d_T,
                                   void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (r && !rev_idx) || (n && (!d_s1 || !d_s2 || !d_rand || !d_o1 || !d_o2 || !d_J || !d_T || (q && !d_msgs))))
        return CC_ERR_DECODE;
    std::vector<uint32_t> idx;
    cc_status s = prove_checks(c, true, q, r, nresp, rev_idx, idx);
    if (s) return s;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    if (c->prove_idx.ensure(idx.size() * 4) || c->prove_scratch.ensure(cck_sigma_prime_words(c->mode, n) * 4))
        return CC_ERR_HIP;
    HIPCK(hipMemcpyAsync(c->prove_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
    return launch_pok_init(c, n, q, r, d_s1, d_s2, d_msgs, c->prove_idx.as<uint32_t>(), d_rand, d_o1, d_o2, d_J, d_T, st);
}

cc_status cc_pok_init_batch(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* s1, const uint8_t* s2,
                            const uint8_t* msgs, const uint64_t* rev_idx, const uint8_t* rand, uint8_t* o1, uint8_t* o2,
                            uint8_t* oJ, uint8_t* oT) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (r && !rev_idx) || (n && (!s1 || !s2 || !rand || !o1 || !o2 || !oJ || !oT || (q && !msgs))))
        return CC_ERR_DECODE;
    std::vector<uint32_t> idx;
    cc_status s = prove_checks(c, true, q, r, nresp, rev_idx, idx);
    if (s) return s;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t sb = (size_t)sig_bytes(c->mode), ob = (size_t)oth_bytes(c->mode), rb = n * (nresp + 2) * 48;
    const size_t scr = cck_sigma_prime_words(c->mode, n) * 4;
    hipStream_t st = c->stream;
    DevBuf &dR = c->in_aux[0], &d1 = c->in_aux[1], &d2 = c->in_aux[2], &dJ = c->in_aux[3], &dT = c->in_aux[4];
    if (c->in_s1.ensure(n * sb) || c->in_s2.ensure(n * sb) || c->in_msgs.ensure(n * q * 48 + 16) || dR.ensure(rb) ||
        d1.ensure(n * sb) || d2.ensure(n * sb) || dJ.ensure(n * ob) || dT.ensure(n * ob) ||
        c->prove_idx.ensure(idx.size() * 4) || c->prove_scratch.ensure(scr))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up(c->in_s1, s1, n * sb);
    f.up(c->in_s2, s2, n * sb);
    f.up(c->in_msgs, msgs, n * q * 48);
    f.up_secret(dR, rand, rb);
    f.up(c->prove_idx, idx.data(), idx.size() * 4);
    f.launch([&] {
        return launch_pok_init(c, n, q, r, c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(), c->in_msgs.as<uint8_t>(),
                               c->prove_idx.as<uint32_t>(), dR.as<uint8_t>(), d1.as<uint8_t>(), d2.as<uint8_t>(),
                               dJ.as<uint8_t>(), dT.as<uint8_t>(), st);
    });
    f.down(o1, d1, n * sb);
    f.down(o2, d2, n * sb);
    f.down(oJ, dJ, n * ob);
    f.down(oT, dT, n * ob);
    // the device copies of the secrets (r1, r2, the blindings; the digits of r1 and r1 r2) are zeroed
    f.wipe(c->prove_scratch, scr);
    return f.finish();
}

cc_status cc_pok_gen_proof_batch_device(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* d_msgs,
                                        const uint64_t* rev_idx, const uint8_t* d_rand, const uint8_t* d_chal,
                                        uint8_t* d_out, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (r && !rev_idx) || (n && (!d_rand || !d_chal || !d_out || (q && !d_msgs)))) return CC_ERR_DECODE;
    std::vector<uint32_t> idx;
    cc_status s = prove_checks(c, false, q, r, nresp, rev_idx, idx);
    if (s) return s;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    if (c->prove_idx.ensure(idx.size() * 4)) return CC_ERR_HIP;
    HIPCK(hipMemcpyAsync(c->prove_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
    KCK(cck_pok_responses(n, (int)q, (int)r, d_msgs, d_rand, d_chal, c->prove_idx.as<uint32_t>(), d_out, st));
    return CC_OK;
}

cc_status cc_pok_gen_proof_batch(cc_ctx* c, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* msgs,
                                 const uint64_t* rev_idx, const uint8_t* rand, const uint8_t* chal, uint8_t* out) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (r && !rev_idx) || (n && (!rand || !chal || !out || (q && !msgs)))) return CC_ERR_DECODE;
    std::vector<uint32_t> idx;
    cc_status s = prove_checks(c, false, q, r, nresp, rev_idx, idx);
    if (s) return s;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t rb = n * (nresp + 2) * 48;
    hipStream_t st = c->stream;
    DevBuf &dR = c->in_aux[0], &dC = c->in_aux[1], &dO = c->in_aux[2];
    if (c->in_msgs.ensure(n * q * 48 + 16) || dR.ensure(rb) || dC.ensure(n * 48) || dO.ensure(n * nresp * 48) ||
        c->prove_idx.ensure(idx.size() * 4))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up(c->in_msgs, msgs, n * q * 48);
    f.up_secret(dR, rand, rb);  // r2 and the blindings
    f.up(dC, chal, n * 48);
    f.up(c->prove_idx, idx.data(), idx.size() * 4);
    f.launch([&] {
        return cck_pok_responses(n, (int)q, (int)r, c->in_msgs.as<uint8_t>(), dR.as<uint8_t>(), dC.as<uint8_t>(),
                                 c->prove_idx.as<uint32_t>(), dO.as<uint8_t>(), st);
    });
    f.down(out, dO, n * nresp * 48);
    return f.finish();
}

cc_status cc_unblind_batch(cc_ctx* c, size_t n, const uint8_t* c1, const uint8_t* c2, const uint8_t* sk,
                           uint8_t* out_sigma2) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!c1 || !c2 || !sk || !out_sigma2))) return CC_ERR_DECODE;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t sb = (size_t)sig_bytes(c->mode);
    const int sg = sig_group(c->mode);
    const size_t scr = n * cck_straus_words(sg, 2) * 4;
    hipStream_t st = c->stream;
    DevBuf &dK = c->in_aux[0], &dP = c->in_aux[1], &dS = c->in_aux[2], &dO = c->in_aux[3];
    if (c->in_s1.ensure(n * sb) || c->in_s2.ensure(n * sb) || dK.ensure(n * 48) || dP.ensure(n * 2 * sb) ||
        dS.ensure(n * 64) || dO.ensure(n * sb))
        return CC_ERR_HIP;
    if (cc_status s = agg_scratch(c, sg, n, 2)) return s;
    HostForm f(st);
    f.up(c->in_s1, c1, n * sb);
    f.up(c->in_s2, c2, n * sb);
    f.up_secret(dK, sk, n * 48);
    f.launch([&]() -> cc_status {
        KCK(cck_unblind_assemble(sg, n, c->in_s1.as<uint8_t>(), c->in_s2.as<uint8_t>(), dK.as<uint8_t>(),
                                 dP.as<uint8_t>(), dS.as<uint32_t>(), st));
        // sigma_2 = c2 + (-sk) c1: one t = 2 Straus task a row (as cc_blind_sign_batch drives it)
        KCK(cck_msm_straus(sg, n, 2, dP.as<uint8_t>(), 2 * sb, 0, sb, dS.as<uint32_t>(), 1,
                           c->agg_scratch.as<uint32_t>(), dO.as<uint8_t>(), st));
        return CC_OK;
    });
    f.down(out_sigma2, dO, n * sb);
    // the device copies of sk, of -sk and of its digits (the Straus scratch) are zeroed
    f.wipe(dS, n * 64);
    f.wipe(c->agg_scratch, scr);
    return f.finish();
}

// ---------------------------------------------------------------- holder side of issuance (sigreq_prove.hip)
// default HBM budget of the request params' tables (at most half of what is free).  The widest
// candidate, 16 bits, takes 0.10 / 0.20 GB a G1 / G2 base, so 4 GiB holds it up to q = 39 / 19.
constexpr double kRqTableBudget = 4.0 * (double)(1ull << 30);

cc_status cc_set_request_params(cc_ctx* c, size_t q, const uint8_t* g, const uint8_t* h, int table_bits) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !g || !h || q == 0 || q > kMaxQ || (table_bits != 0 && (table_bits < 8 || table_bits > 16)))
        return CC_ERR_DECODE;
    // no request params until every step below has succeeded (as cc_set_issuers)
    c->have_rq = false;
    c->rq_q = 0;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches before the tables are rebuilt
    HIPCK(hipStreamSynchronize(c->stream));  // an asynchronous *_device call may still read the old tables
    const int sg = sig_group(c->mode);
    const size_t sb = (size_t)sig_bytes(c->mode), aw = aff_words(sg), nb = q + 1;
    std::vector<uint8_t> enc(nb * sb);  // [h_0 .. h_{q-1}, g]: g is table base q
    memcpy(enc.data(), h, q * sb);
    memcpy(enc.data() + q * sb, g, sb);
    c->rq_table.release();
    auto tbytes = [&](int w) { return nb * tab_words(sg, w) * 4; };
    int wb = pick_table_bits(table_bits, kRqTableBudget, tbytes);
    if (c->rq_aff.ensure(nb * aw * 4) || c->rq_inf.ensure(nb * 4)) return CC_ERR_HIP;
    wb = alloc_tables(wb, table_bits != 0, tbytes, [&](int w) { return c->rq_table.ensure(tbytes(w)) == 0; });
    if (!wb) return CC_ERR_HIP;
    cc_status s = decode_points_host(c, sg, nb, enc.data(), c->rq_aff.as<uint32_t>(), c->rq_inf.as<uint32_t>());
    if (s) return s;
    DevBuf pw;
    if (pw.ensure(nb * tab_nwin(wb) * (sg == 1 ? 36 : 72) * 4)) return CC_ERR_HIP;
    // lazy form: the sums read the tables through ft_add_lz / pl::ft_add_g2_lz
    KCK(cck_build_table(sg, (int)nb, wb, c->rq_aff.as<uint32_t>(), c->rq_inf.as<uint32_t>(), pw.as<uint32_t>(),
                        c->rq_table.as<uint32_t>(), 1, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->rq_q = q;
    c->rq_wbits = wb;
    c->have_rq = true;
    return CC_OK;
}

static cc_status rq_ensure_two(cc_ctx* c, size_t n, size_t k) {
    if (!k) return CC_OK;
    if (c->rq_tab.ensure(cck_rq_table_words(sig_group(c->mode), n) * 4) ||
        c->rq_dig.ensure(cck_rq_digit_bytes(n, (int)k)))
        return CC_ERR_HIP;
    return CC_OK;
}

static cc_status launch_sigreq_new(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_msgs, const uint8_t* d_pk,
                                   const uint8_t* d_rand, uint8_t* d_comm, uint8_t* d_h, uint8_t* d_cts,
                                   hipStream_t st) {
    const int sg = sig_group(c->mode);
    const size_t len = (size_t)sig_bytes(c->mode) + 48 * (q - k);
    if (c->rq_hdata.ensure(n * len + 16) || c->rq_hoff.ensure((n + 1) * 8) || c->rq_fail.ensure(4)) return CC_ERR_HIP;
    cc_status s = rq_ensure_two(c, n, k);
    if (s) return s;
    KCK(cck_rq_fixed(sg, n, (int)q, (int)k, 0, d_msgs, d_rand, c->rq_table.as<uint32_t>(), c->rq_wbits,
                     c->rq_inf.as<uint32_t>(), d_comm, d_cts, st));
    // h = compute_h(commitment, known) as cc_blind_sign_batch computes it (compute_h_batch), rows built on
    // the device
    KCK(cck_rq_h_rows(sg, n, (int)q, (int)k, d_comm, d_msgs, c->rq_hdata.as<uint8_t>(), c->rq_hoff.as<uint64_t>(), st));
    HIPCK(hipMemsetAsync(c->rq_fail.p, 0, 4, st));
    KCK(cck_h_input_canon(sg, n, len, (int)(q - k), c->rq_hdata.as<uint8_t>(), st));
    KCK(cck_hash_to_curve(sg, n, c->rq_hdata.as<uint8_t>(), c->rq_hoff.as<uint64_t>(), d_h, c->rq_fail.as<uint32_t>(),
                          st));
    KCK(cck_rq_two_base(sg, n, (int)q, (int)k, 0, d_pk, d_h, d_msgs, d_rand, c->rq_tab.as<uint32_t>(),
                        c->rq_dig.as<int8_t>(), d_cts, st));
    return CC_OK;
}

cc_status cc_sigreq_new_batch_device(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_msgs,
                                     const uint8_t* d_pk, const uint8_t* d_rand, uint8_t* d_comm, uint8_t* d_h,
                                     uint8_t* d_cts, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_rand || !d_comm || !d_h || (q && !d_msgs) || (k && (!d_pk || !d_cts))))) return CC_ERR_DECODE;
    cc_status s = rq_checks(c, true, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    return launch_sigreq_new(c, n, q, k, d_msgs, d_pk, d_rand, d_comm, d_h, d_cts, st);
}

cc_status cc_sigreq_new_batch(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* msgs, const uint8_t* pk,
                              const uint8_t* rand, uint8_t* out_comm, uint8_t* out_h, uint8_t* out_cts) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!rand || !out_comm || !out_h || (q && !msgs) || (k && (!pk || !out_cts))))) return CC_ERR_DECODE;
    cc_status s = rq_checks(c, true, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t sb = (size_t)sig_bytes(c->mode), rb = n * (k + 1) * 48, mb = n * q * 48;
    hipStream_t st = c->stream;
    DevBuf &dR = c->in_aux[0], &dP = c->in_aux[1], &dC = c->in_aux[2], &dH = c->in_aux[3], &dT = c->in_aux[4];
    if (c->in_msgs.ensure(mb + 16) || dR.ensure(rb) || dP.ensure(n * sb) || dC.ensure(n * sb) || dH.ensure(n * sb) ||
        dT.ensure(n * k * 2 * sb + 16))
        return CC_ERR_HIP;
    s = rq_ensure_two(c, n, k);  // before the launch: the wipe covers the digits of this call
    if (s) return s;
    uint32_t fail = 0;
    HostForm f(st);
    f.up_secret(c->in_msgs, msgs, mb);
    f.up_secret(dR, rand, rb);
    f.up(dP, pk, k ? n * sb : 0);
    f.launch([&] {
        return launch_sigreq_new(c, n, q, k, c->in_msgs.as<uint8_t>(), dP.as<uint8_t>(), dR.as<uint8_t>(),
                                 dC.as<uint8_t>(), dH.as<uint8_t>(), dT.as<uint8_t>(), st);
    });
    f.down(out_comm, dC, n * sb);
    f.down(out_h, dH, n * sb);
    f.down(out_cts, dT, n * k * 2 * sb);
    f.down(&fail, c->rq_fail, 4);
    // the device copies of the secrets (the messages, r and the k_i, the digits of k_i and m_i) are zeroed
    f.wipe(c->rq_dig, k ? cck_rq_digit_bytes(n, (int)k) : 0);
    s = f.finish();
    if (!s && fail) return CC_ERR_DECODE;  // as cc_hash_to_curve: 4,096 failed tries
    return s;
}

static cc_status launch_sigreq_init(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_h, const uint8_t* d_pk,
                                    const uint8_t* d_blind, uint8_t* d_proofs, hipStream_t st) {
    const int sg = sig_group(c->mode);
    cc_status s = rq_ensure_two(c, n, k);
    if (s) return s;
    HIPCK(hipMemsetAsync(d_proofs, 0, n * cck_sigreq_proof_bytes(sg, (int)k), st));  // the response fields
    KCK(cck_rq_fixed(sg, n, (int)q, (int)k, 1, nullptr, d_blind, c->rq_table.as<uint32_t>(), c->rq_wbits,
                     c->rq_inf.as<uint32_t>(), d_proofs, d_proofs, st));
    KCK(cck_rq_two_base(sg, n, (int)q, (int)k, 1, d_pk, d_h, nullptr, d_blind, c->rq_tab.as<uint32_t>(),
                        c->rq_dig.as<int8_t>(), d_proofs, st));
    return CC_OK;
}

cc_status cc_sigreq_pok_init_batch_device(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_h,
                                          const uint8_t* d_pk, const uint8_t* d_blind, uint8_t* d_proofs,
                                          void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_blind || !d_proofs || (k && (!d_h || !d_pk))))) return CC_ERR_DECODE;
    cc_status s = rq_checks(c, true, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    return launch_sigreq_init(c, n, q, k, d_h, d_pk, d_blind, d_proofs, st);
}

cc_status cc_sigreq_pok_init_batch(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* h, const uint8_t* pk,
                                   const uint8_t* blind, uint8_t* out_proofs) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!blind || !out_proofs || (k && (!h || !pk))))) return CC_ERR_DECODE;
    cc_status s = rq_checks(c, true, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t sb = (size_t)sig_bytes(c->mode), bb = n * (3 * k + 2) * 48;
    const size_t pb = n * cck_sigreq_proof_bytes(sig_group(c->mode), (int)k);
    hipStream_t st = c->stream;
    DevBuf &dB = c->in_aux[0], &dP = c->in_aux[1], &dH = c->in_aux[2], &dO = c->in_aux[3];
    if (dB.ensure(bb) || dP.ensure(n * sb) || dH.ensure(n * sb) || dO.ensure(pb)) return CC_ERR_HIP;
    s = rq_ensure_two(c, n, k);
    if (s) return s;
    HostForm f(st);
    f.up_secret(dB, blind, bb);
    f.up(dP, pk, k ? n * sb : 0);
    f.up(dH, h, k ? n * sb : 0);
    f.launch([&] {
        return launch_sigreq_init(c, n, q, k, dH.as<uint8_t>(), dP.as<uint8_t>(), dB.as<uint8_t>(), dO.as<uint8_t>(), st);
    });
    f.down(out_proofs, dO, pb);
    // the device copies of the blindings and of the digits of b2_i and hb_i are zeroed
    f.wipe(c->rq_dig, k ? cck_rq_digit_bytes(n, (int)k) : 0);
    return f.finish();
}

cc_status cc_sigreq_pok_gen_proof_batch_device(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_msgs,
                                               const uint8_t* d_rand, const uint8_t* d_blind, const uint8_t* d_sk,
                                               const uint8_t* d_chal, uint8_t* d_proofs, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_rand || !d_blind || !d_sk || !d_chal || !d_proofs || (k && !d_msgs)))) return CC_ERR_DECODE;
    cc_status s = rq_checks(c, false, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    KCK(cck_rq_responses(sig_group(c->mode), n, (int)q, (int)k, d_msgs, d_rand, d_blind, d_sk, d_chal, d_proofs, st));
    return CC_OK;
}

cc_status cc_sigreq_pok_gen_proof_batch(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* msgs,
                                        const uint8_t* rand, const uint8_t* blind, const uint8_t* sk,
                                        const uint8_t* chal, uint8_t* proofs) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!rand || !blind || !sk || !chal || !proofs || (k && !msgs)))) return CC_ERR_DECODE;
    cc_status s = rq_checks(c, false, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t rb = n * (k + 1) * 48, bb = n * (3 * k + 2) * 48, mb = n * q * 48;
    const size_t pb = n * cck_sigreq_proof_bytes(sig_group(c->mode), (int)k);
    hipStream_t st = c->stream;
    DevBuf &dR = c->in_aux[0], &dB = c->in_aux[1], &dK = c->in_aux[2], &dC = c->in_aux[3], &dO = c->in_aux[4];
    if (c->in_msgs.ensure(mb + 16) || dR.ensure(rb) || dB.ensure(bb) || dK.ensure(n * 48) || dC.ensure(n * 48) ||
        dO.ensure(pb))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up_secret(c->in_msgs, msgs, k ? mb : 0);
    f.up_secret(dR, rand, rb);
    f.up_secret(dB, blind, bb);
    f.up_secret(dK, sk, n * 48);
    f.up(dC, chal, n * 48);
    f.up(dO, proofs, pb);
    f.launch([&] {
        return cck_rq_responses(sig_group(c->mode), n, (int)q, (int)k, c->in_msgs.as<uint8_t>(), dR.as<uint8_t>(),
                                dB.as<uint8_t>(), dK.as<uint8_t>(), dC.as<uint8_t>(), dO.as<uint8_t>(), st);
    });
    f.down(proofs, dO, pb);
    return f.finish();  // zeroes the device copies of the messages, r and the k_i, the blindings and the ElGamal key
}
