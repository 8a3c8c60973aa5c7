// C ABI, issuer side: subgroup checks, hash-to-curve, blind signing, request-proof and VSS verify, and the
// device forms of issue_dev.hip (ctx.h).
#include "ctx.h"

// ---------------------------------------------------------------- codec: subgroup membership (§8(f) row 1)
cc_status cc_subgroup_check(cc_ctx* c, int group, size_t n, const uint8_t* points, uint8_t* status) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (group != 1 && group != 2) || (n && (!points || !status))) return CC_ERR_DECODE;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    return subgroup_host(c, group, n, points, status);
}

// ---------------------------------------------------------------- hash-to-curve (§8(f) row 2)
// the checks of a message list (data, offsets[n + 1]) and its device buffers; the caller uploads
// offsets[n] bytes of data and the n + 1 offsets
static cc_status stage_messages(size_t n, const uint8_t* data, const uint64_t* offsets, DevBuf& d_data, DevBuf& d_off) {
    if (offsets[0] != 0) return CC_ERR_DECODE;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return CC_ERR_DECODE;
    const size_t total = offsets[n];
    if (total && !data) return CC_ERR_DECODE;
    if (d_data.ensure(total + 16) || d_off.ensure((n + 1) * 8)) return CC_ERR_HIP;
    return CC_OK;
}

// from_msg_hash of the n messages (data, offsets[n + 1]) into d_out, and to host_out if given.  canon_len != 0: the
// rows are compute_h inputs of that length with kn known messages; the reference hashes commitment.to_bytes() and
// the known messages' to_bytes(), so they are made canonical first.
static cc_status hash_rows(cc_ctx* c, int group, size_t n, const uint8_t* data, const uint64_t* offsets, size_t canon_len,
                           int kn, DevBuf& d_out, uint8_t* host_out) {
    const size_t eb = group == 1 ? 97 : 192;
    DevBuf d_data, d_off, d_fail;
    cc_status s = stage_messages(n, data, offsets, d_data, d_off);
    if (s) return s;
    if (d_out.ensure(n * eb) || d_fail.ensure(4)) return CC_ERR_HIP;
    uint32_t fail = 0;
    HostForm f(c->stream);
    f.up(d_data, data, offsets[n]);
    f.up(d_off, offsets, (n + 1) * 8);
    f.launch([&]() -> cc_status {
        HIPCK(hipMemsetAsync(d_fail.p, 0, 4, c->stream));
        if (canon_len) KCK(cck_h_input_canon(group, n, canon_len, kn, d_data.as<uint8_t>(), c->stream));
        KCK(cck_hash_to_curve(group, n, d_data.as<uint8_t>(), d_off.as<uint64_t>(), d_out.as<uint8_t>(),
                              d_fail.as<uint32_t>(), c->stream));
        return CC_OK;
    });
    f.down(host_out, d_out, host_out ? n * eb : 0);
    f.down(&fail, d_fail, 4);
    s = f.finish();
    if (s) return s;
    return fail ? CC_ERR_DECODE : CC_OK;  // 4,096 failed tries (probability ~2^-4096)
}

cc_status cc_hash_to_curve(cc_ctx* c, int group, size_t n, const uint8_t* data, const uint64_t* offsets, uint8_t* out) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (group != 1 && group != 2) || (n && (!offsets || !out))) return CC_ERR_DECODE;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    DevBuf d_out;
    return hash_rows(c, group, n, data, offsets, 0, 0, d_out, out);
}

cc_status cc_hash_msg(cc_ctx* c, size_t n, const uint8_t* data, const uint64_t* offsets, uint8_t* out48) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!offsets || !out48))) return CC_ERR_DECODE;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    DevBuf d_data, d_off, d_out;
    cc_status s = stage_messages(n, data, offsets, d_data, d_off);
    if (s) return s;
    if (d_out.ensure(n * 48)) return CC_ERR_HIP;
    HostForm f(c->stream);
    f.up(d_data, data, offsets[n]);
    f.up(d_off, offsets, (n + 1) * 8);
    f.launch([&] {
        return cck_shake256_48(n, d_data.as<uint8_t>(), d_off.as<uint64_t>(), d_out.as<uint8_t>(), c->stream);
    });
    f.down(out48, d_out, n * 48);
    return f.finish();
}

// ---------------------------------------------------------------- issuance (§8(f) row 3)
// h_r = compute_h(commitment_r, known_r) for every request, on the device (hash.hip)
static cc_status compute_h_batch(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* comm, const uint8_t* known,
                                 DevBuf& d_h) {
    const size_t sb = (size_t)sig_bytes(c->mode), kn = q - k, len = sb + 48 * kn;
    std::vector<uint8_t> data(n * len);
    std::vector<uint64_t> off(n + 1);
    for (size_t r = 0; r < n; r++) {
        memcpy(&data[r * len], comm + r * sb, sb);
        if (kn) memcpy(&data[r * len + sb], known + r * kn * 48, kn * 48);
        off[r] = r * len;
    }
    off[n] = n * len;
    return hash_rows(c, sig_group(c->mode), n, data.data(), off.data(), len, (int)kn, d_h, nullptr);
}

cc_status cc_blind_sign_batch(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* commitment, const uint8_t* known,
                              const uint8_t* ciphertexts, const uint8_t* x, const uint8_t* y, uint8_t* out_h,
                              uint8_t* out_c1, uint8_t* out_c2) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !x || (q && !y) || (n && (!commitment || !out_h || !out_c1 || !out_c2 || (k && !ciphertexts) ||
                                        (q > k && !known))))
        return CC_ERR_DECODE;
    if (q > kMaxQ) return CC_ERR_DECODE;
    if (k > q) return CC_ERR_LEN;  // reference: hidden + known == y.len() (assert_eq!)
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    const size_t sb = (size_t)sig_bytes(c->mode), t = k + 1;
    const int sg = sig_group(c->mode);
    hipStream_t st = c->stream;
    DevBuf d_h, d_cts, d_known, d_x, d_y, d_pts, d_sc, d_out;
    cc_status s = compute_h_batch(c, n, q, k, commitment, known, d_h);
    if (s) return s;
    if (d_cts.ensure(n * k * 2 * sb + 16) || d_known.ensure(n * (q - k) * 48 + 16) || d_x.ensure(48) ||
        d_y.ensure(q * 48 + 16) || d_pts.ensure(2 * n * t * sb) || d_sc.ensure(2 * n * t * 32) ||
        d_out.ensure(2 * n * sb))
        return CC_ERR_HIP;
    s = agg_scratch(c, sg, 2 * n, t);
    if (s) return s;
    const size_t scr = 2 * n * cck_straus_words(sg, t) * 4;
    std::vector<uint8_t> o(2 * n * sb);
    HostForm f(st);
    f.up(d_cts, ciphertexts, n * k * 2 * sb);
    f.up(d_known, known, n * (q - k) * 48);
    f.up_secret(d_x, x, 48);
    f.up_secret(d_y, y, q * 48);
    f.launch([&]() -> cc_status {
        KCK(cck_blind_assemble(sg, n, (int)q, (int)k, d_cts.as<uint8_t>(), d_h.as<uint8_t>(), d_known.as<uint8_t>(),
                               d_x.as<uint8_t>(), d_y.as<uint8_t>(), d_pts.as<uint8_t>(), d_sc.as<uint32_t>(), st));
        KCK(cck_msm_straus(sg, 2 * n, t, d_pts.as<uint8_t>(), t * sb, 0, sb, d_sc.as<uint32_t>(), 1,
                           c->agg_scratch.as<uint32_t>(), d_out.as<uint8_t>(), st));
        return CC_OK;
    });
    f.down(o.data(), d_out, 2 * n * sb);
    f.down(out_h, d_h, n * sb);
    // the device copies of x and y, of the tasks' scalars (y_i, x + sum y m) and of their digits (the Straus
    // scratch) are zeroed, as cc_blind_sign_batch_device zeroes its own
    f.wipe(d_sc, 2 * n * t * 32);
    f.wipe(c->agg_scratch, scr);
    s = f.finish();
    if (s) return s;
    for (size_t r = 0; r < n; r++) {
        memcpy(out_c1 + r * sb, &o[(2 * r) * sb], sb);
        memcpy(out_c2 + r * sb, &o[(2 * r + 1) * sb], sb);
    }
    return CC_OK;
}

size_t cc_sigreq_proof_bytes(const cc_ctx* c, size_t k) {
    c = primary(c);
    return c ? cck_sigreq_proof_bytes(sig_group(c->mode), (int)k) : 0;
}

cc_status cc_sigreq_verify_batch(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* g, const uint8_t* hvec,
                                 const uint8_t* commitment, const uint8_t* known, const uint8_t* ciphertexts,
                                 const uint8_t* elgamal_pk, const uint8_t* proofs, const uint8_t* chal,
                                 uint8_t* verdicts) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !g || (k && !hvec) ||
        (n && (!commitment || !elgamal_pk || !proofs || !chal || !verdicts || (k && !ciphertexts) || (q > k && !known))))
        return CC_ERR_DECODE;
    if (q > kMaxQ) return CC_ERR_DECODE;
    if (k > q) return CC_ERR_LEN;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    const size_t sb = (size_t)sig_bytes(c->mode);
    const int sg = sig_group(c->mode);
    const size_t pb = cck_sigreq_proof_bytes(sg, (int)k);
    hipStream_t st = c->stream;
    DevBuf d_h, d_g, d_hv, d_comm, d_cts, d_pk, d_pr, d_ch, d_scr, d_ok, d_v;
    cc_status s = compute_h_batch(c, n, q, k, commitment, known, d_h);
    if (s) return s;
    if (d_g.ensure(sb) || d_hv.ensure(k * sb + 16) || d_comm.ensure(n * sb) || d_cts.ensure(n * k * 2 * sb + 16) ||
        d_pk.ensure(n * sb) || d_pr.ensure(n * pb) || d_ch.ensure(n * 48) ||
        d_scr.ensure(cck_sigreq_scratch_words(sg, n, (int)k) * 4) || d_ok.ensure(n * (2 + 2 * k)) || d_v.ensure(n))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up(d_g, g, sb);
    f.up(d_hv, hvec, k * sb);
    f.up(d_comm, commitment, n * sb);
    f.up(d_cts, ciphertexts, n * k * 2 * sb);
    f.up(d_pk, elgamal_pk, n * sb);
    f.up(d_pr, proofs, n * pb);
    f.up(d_ch, chal, n * 48);
    f.launch([&] {
        return cck_sigreq_verify(sg, n, (int)k, d_g.as<uint8_t>(), d_hv.as<uint8_t>(), d_comm.as<uint8_t>(),
                                 d_cts.as<uint8_t>(), d_pk.as<uint8_t>(), d_pr.as<uint8_t>(), d_ch.as<uint8_t>(),
                                 d_h.as<uint8_t>(), d_scr.as<uint32_t>(), d_ok.as<uint8_t>(), d_v.as<uint8_t>(), st);
    });
    f.down(verdicts, d_v, n);
    return f.finish();
}

// ---------------------------------------------------------------- keygen: Pedersen VSS (§8(f) row 4)
cc_status cc_vss_verify_batch(cc_ctx* c, size_t n, size_t t, const uint8_t* g, const uint8_t* h,
                              const uint8_t* commitments, size_t n_sets, const uint32_t* set_of, const uint64_t* ids,
                              const uint8_t* shares, uint8_t* verdicts) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !g || !h || (n && (!commitments || !set_of || !ids || !shares || !verdicts)) || t == 0 || t > 4096 ||
        n > kMaxBatch || n_sets > kMaxBatch)
        return CC_ERR_DECODE;
    for (size_t i = 0; i < n; i++)
        if (set_of[i] >= n_sets) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf d_g, d_h, d_c, d_set, d_ids, d_sh, d_scr, d_ok;
    if (d_g.ensure(97) || d_h.ensure(97) || d_c.ensure(n_sets * t * 97) || d_set.ensure(n * 4) || d_ids.ensure(n * 8) ||
        d_sh.ensure(n * 96) || d_scr.ensure(n * (t + 2) * 33 * 4) || d_ok.ensure(n))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up(d_g, g, 97);
    f.up(d_h, h, 97);
    f.up(d_c, commitments, n_sets * t * 97);
    f.up(d_set, set_of, n * 4);
    f.up(d_ids, ids, n * 8);
    f.up(d_sh, shares, n * 96);
    f.launch([&] {
        return cck_vss_verify(n, (int)t, d_g.as<uint8_t>(), d_h.as<uint8_t>(), d_c.as<uint8_t>(), d_set.as<uint32_t>(),
                              d_ids.as<uint64_t>(), d_sh.as<uint8_t>(), d_scr.as<uint32_t>(), d_ok.as<uint8_t>(), st);
    });
    f.down(verdicts, d_ok, n);
    return f.finish();
}

// ---------------------------------------------------------------- issuer side, device forms (issue_dev.hip)
// h = compute_h(commitment, known) as compute_h_batch computes it, rows built on the device.  The one-in-
// 2^4096 failure of the hash is not reported (as cc_sigreq_new_batch_device).
static cc_status launch_issuer_h(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_comm, const uint8_t* d_known,
                                 uint8_t* d_h, hipStream_t st) {
    const int sg = sig_group(c->mode);
    const size_t kn = q - k, len = (size_t)sig_bytes(c->mode) + 48 * kn;
    if (c->rq_hdata.ensure(n * len + 16) || c->rq_hoff.ensure((n + 1) * 8) || c->rq_fail.ensure(4)) return CC_ERR_HIP;
    // the known messages are the rows' only messages: q - k of them, none hidden
    KCK(cck_rq_h_rows(sg, n, (int)kn, 0, d_comm, d_known, c->rq_hdata.as<uint8_t>(), c->rq_hoff.as<uint64_t>(), st));
    HIPCK(hipMemsetAsync(c->rq_fail.p, 0, 4, st));
    KCK(cck_h_input_canon(sg, n, len, (int)kn, c->rq_hdata.as<uint8_t>(), st));
    KCK(cck_hash_to_curve(sg, n, c->rq_hdata.as<uint8_t>(), c->rq_hoff.as<uint64_t>(), d_h, c->rq_fail.as<uint32_t>(),
                          st));
    return CC_OK;
}

cc_status cc_sigreq_verify_batch_device(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_commitment,
                                        const uint8_t* d_known, const uint8_t* d_ciphertexts,
                                        const uint8_t* d_elgamal_pk, const uint8_t* d_proofs, const uint8_t* d_chal,
                                        uint8_t* d_verdicts, uint8_t* d_out_h, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_commitment || !d_elgamal_pk || !d_proofs || !d_chal || !d_verdicts || (k && !d_ciphertexts) ||
                     (q > k && !d_known))))
        return CC_ERR_DECODE;
    cc_status s = rq_checks(c, true, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    const int sg = sig_group(c->mode);
    if (!d_out_h) {
        if (c->iv_h.ensure(n * (size_t)sig_bytes(c->mode))) return CC_ERR_HIP;
        d_out_h = c->iv_h.as<uint8_t>();
    }
    if (c->iv_tab.ensure(cck_iv_table_words(sg, n, (int)k) * 4) || c->iv_cdig.ensure(cck_iv_cdig_bytes(n)) ||
        c->iv_dig.ensure(cck_iv_dig_bytes(n, (int)k) + 16) || c->iv_ok.ensure(cck_iv_ok_bytes(n, (int)k)))
        return CC_ERR_HIP;
    s = launch_issuer_h(c, n, q, k, d_commitment, d_known, d_out_h, st);
    if (s) return s;
    KCK(cck_iv_checks(sg, n, (int)q, (int)k, d_commitment, d_ciphertexts, d_elgamal_pk, d_proofs, d_chal, d_out_h,
                      c->rq_table.as<uint32_t>(), c->rq_wbits, c->rq_inf.as<uint32_t>(), c->iv_tab.as<uint32_t>(),
                      c->iv_cdig.as<int8_t>(), c->iv_dig.as<int8_t>(), c->iv_ok.as<uint8_t>(), st));
    KCK(cck_sigreq_combine(sg, n, (int)k, d_proofs, c->iv_ok.as<uint8_t>(), d_verdicts, st));
    return CC_OK;
}

cc_status cc_blind_sign_batch_device(cc_ctx* c, size_t n, size_t q, size_t k, const uint8_t* d_commitment,
                                     const uint8_t* d_known, const uint8_t* d_ciphertexts, const uint8_t* d_h,
                                     const uint8_t* x, const uint8_t* y, uint8_t* d_out_h, uint8_t* d_out_c1,
                                     uint8_t* d_out_c2, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !x || (q && !y) ||
        (n && ((!d_h && !d_commitment) || !d_out_h || !d_out_c1 || !d_out_c2 || (k && !d_ciphertexts) ||
               (q > k && !d_known))))
        return CC_ERR_DECODE;
    cc_status s = rq_checks(c, false, n, q, k);
    if (s) return s;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    const size_t sb = (size_t)sig_bytes(c->mode), t = k + 1, xyb = (q + 1) * 48;
    const int sg = sig_group(c->mode);
    if (c->bs_pts.ensure(2 * n * t * sb) || c->bs_sc.ensure(2 * n * t * 32) || c->bs_out.ensure(2 * n * sb) ||
        c->bs_xy.ensure(xyb + 16))
        return CC_ERR_HIP;
    s = agg_scratch(c, sg, 2 * n, t);
    if (s) return s;
    const size_t scr = 2 * n * cck_straus_words(sg, t) * 4;
    if (d_h) {
        if (d_h != d_out_h) HIPCK(hipMemcpyAsync(d_out_h, d_h, n * sb, hipMemcpyDeviceToDevice, st));
    } else {
        s = launch_issuer_h(c, n, q, k, d_commitment, d_known, d_out_h, st);
        if (s) return s;
    }
    HostForm f(st, /*sync=*/false);  // a device form: the work and the wipes stay queued on the caller's stream
    f.launch([&]() -> cc_status {
        // x | y through the pinned ring: the caller's arrays are free again when the call returns
        std::vector<uint8_t> xy(xyb);
        memcpy(xy.data(), x, 48);
        if (q) memcpy(xy.data() + 48, y, q * 48);
        const int up = c->stage[0].upload(c->dev, c->bs_xy.p, xy.data(), xyb, st);
        std::fill(xy.begin(), xy.end(), (uint8_t)0);
        if (up) return CC_ERR_HIP;
        KCK(cck_blind_assemble(sg, n, (int)q, (int)k, d_ciphertexts, d_out_h, d_known, c->bs_xy.as<uint8_t>(),
                               c->bs_xy.as<uint8_t>() + 48, c->bs_pts.as<uint8_t>(), c->bs_sc.as<uint32_t>(), st));
        KCK(cck_msm_straus(sg, 2 * n, t, c->bs_pts.as<uint8_t>(), t * sb, 0, sb, c->bs_sc.as<uint32_t>(), 1,
                           c->agg_scratch.as<uint32_t>(), c->bs_out.as<uint8_t>(), st));
        // tasks 2r / 2r + 1 -> c~1_r / c~2_r: strided device copies
        KCK(cck_copy_rows(n, sb, c->bs_out.as<uint8_t>(), 2 * sb, d_out_c1, st));
        KCK(cck_copy_rows(n, sb, c->bs_out.as<uint8_t>() + sb, 2 * sb, d_out_c2, st));
        return CC_OK;
    });
    // queued behind the work: the device copies of x | y, of the tasks' scalars (y_i, x + sum y m) and of
    // their digits (the Straus scratch) are zeroed
    f.wipe(c->bs_xy, xyb);
    f.wipe(c->bs_sc, 2 * n * t * 32);
    f.wipe(c->agg_scratch, scr);
    return f.finish();
}
