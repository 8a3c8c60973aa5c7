// C ABI, aggregation: Signature::aggregate and Verkey::aggregate over host and device arrays, the issuer
// table and its ids forms, cc_fixed_base_mul (ctx.h).
#include "ctx.h"

// Lagrange-weighted MSMs: windowed Straus over variable bases (aggregate.hip k_msm_straus)
cc_status cc::host::agg_scratch(cc_ctx* c, int group, size_t ntask, size_t t) {
    return c->agg_scratch.ensure(ntask * cck_straus_words(group, t) * 4 + 64) ? CC_ERR_HIP : CC_OK;
}

// the aggregation forms' checks after the NULL checks, in the header's order; the reference asserts
// sigs.len() >= threshold and reads sigs[0] (signature.rs:449-452)
static cc_status agg_checks(size_t n, size_t len, size_t t) {
    if (len > kMaxIds) return CC_ERR_DECODE;
    if (len < t || len == 0) return CC_ERR_THRESHOLD;
    return n > kMaxBatch ? CC_ERR_DECODE : CC_OK;
}

static cc_status launch_sig_aggregate(cc_ctx* c, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                      const uint8_t* d_s1, const uint8_t* d_s2, uint8_t* d_o1, uint8_t* d_o2,
                                      hipStream_t st) {
    const size_t sb = (size_t)sig_bytes(c->mode);
    const int sg = sig_group(c->mode);
    if (c->lag.ensure(n * t * 32 + 32)) return CC_ERR_HIP;
    cc_status s = agg_scratch(c, sg, n, t);
    if (s) return s;
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
    KCK(cck_lagrange(n, len, t, d_ids, c->lag.as<uint32_t>(), st));
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    KCK(cck_msm_straus(sg, n, t, d_s2, len * sb, 0, sb, c->lag.as<uint32_t>(), 1, c->agg_scratch.as<uint32_t>(), d_o2, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    // sigma_1 = sigs[0].sigma_1 (signature.rs:452): strided device copy of entry 0
    KCK(cck_copy_rows(n, sb, d_s1, len * sb, d_o1, st));
    if (c->timing) (void)hipEventRecord(c->ev[3], st);
    return CC_OK;
}

static cc_status launch_vk_aggregate_ids(cc_ctx* c, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                         uint8_t* d_oX, uint8_t* d_oY, hipStream_t st) {
    if (c->lag.ensure(n * t * 32 + 32)) return CC_ERR_HIP;
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
    KCK(cck_lagrange(n, len, t, d_ids, c->lag.as<uint32_t>(), st));
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    if (!c->dev_err.p) {  // sticky until cc_device_error reads it
        if (c->dev_err.ensure(4)) return CC_ERR_HIP;
        HIPCK(hipMemsetAsync(c->dev_err.p, 0, 4, st));
    }
    KCK(cck_vk_agg_fixed(oth_group(c->mode), n, len, t, (int)c->iss_q, d_ids, c->lag.as<uint32_t>(),
                         c->iss_ids.as<uint64_t>(), (int)c->iss_n, c->iss_table.as<uint32_t>(), c->iss_wbits,
                         c->iss_inf.as<uint32_t>(), d_oX, d_oY, c->dev_err.as<uint32_t>(), st));
    if (c->timing) {
        (void)hipEventRecord(c->ev[2], st);
        (void)hipEventRecord(c->ev[3], st);
    }
    return CC_OK;
}

cc_status cc_fixed_base_mul(cc_ctx* c, int group, const uint8_t* base, size_t n, const uint8_t* scalars,
                            uint8_t* out) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || !base || (n && (!scalars || !out)) || (group != 1 && group != 2)) return CC_ERR_DECODE;
    if (n > kMaxBatch) return CC_ERR_DECODE;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    size_t eb = group == 1 ? 97 : 192, aw = aff_words(group);
    hipStream_t st = c->stream;
    DevBuf aff, inf, pw, table, ks, o;
    if (aff.ensure(aw * 4) || inf.ensure(4) || pw.ensure(tab_nwin(8) * (group == 1 ? 36 : 72) * 4) ||
        table.ensure(tab_words(group, 8) * 4) || ks.ensure(n * 48) || o.ensure(n * eb))
        return CC_ERR_HIP;
    cc_status s = decode_points_host(c, group, 1, base, aff.as<uint32_t>(), inf.as<uint32_t>());
    if (s) return s;
    uint32_t binf = 0;
    HIPCK(hipMemcpy(&binf, inf.p, 4, hipMemcpyDeviceToHost));
    HostForm f(st);
    f.up(ks, scalars, n * 48);
    f.launch([&]() -> cc_status {
        KCK(cck_build_table(group, 1, 8, aff.as<uint32_t>(), inf.as<uint32_t>(), pw.as<uint32_t>(), table.as<uint32_t>(),
                            0, st));
        KCK(cck_fixed_mul(group, n, ks.as<uint8_t>(), table.as<uint32_t>(), binf, o.as<uint8_t>(), st));
        return CC_OK;
    });
    f.down(out, o, n * eb);
    return f.finish();
}

cc_status cc_signature_aggregate_batch_device(cc_ctx* c, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                              const uint8_t* d_s1, const uint8_t* d_s2, uint8_t* d_out_s1,
                                              uint8_t* d_out_s2, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_ids || !d_s1 || !d_s2 || !d_out_s1 || !d_out_s2))) return CC_ERR_DECODE;
    if (cc_status e = agg_checks(n, len, t)) return e;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    cc_status s = launch_sig_aggregate(c, n, len, t, d_ids, d_s1, d_s2, d_out_s1, d_out_s2, st);
    if (s) return s;
    if (c->timing) collect_timing(c);
    return CC_OK;
}

cc_status cc_signature_aggregate_batch(cc_ctx* c, size_t n, size_t len, size_t t, const uint64_t* ids,
                                       const uint8_t* s1, const uint8_t* s2, uint8_t* out_s1, uint8_t* out_s2) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!ids || !s1 || !s2 || !out_s1 || !out_s2))) return CC_ERR_DECODE;
    if (cc_status e = agg_checks(n, len, t)) return e;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    size_t sb = (size_t)sig_bytes(c->mode);
    hipStream_t st = c->stream;
    DevBuf &d_ids = c->in_aux[0], &d_pts = c->in_aux[1], &d_out = c->in_aux[2], &d_p1 = c->in_aux[3],
           &d_o1 = c->in_aux[4];
    if (d_ids.ensure(n * len * 8) || d_pts.ensure(n * len * sb) || d_out.ensure(n * sb) || d_p1.ensure(n * len * sb) ||
        d_o1.ensure(n * sb))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up(d_ids, ids, n * len * 8);
    f.up(d_pts, s2, n * len * sb);
    f.up(d_p1, s1, n * len * sb);
    f.launch([&] {
        return launch_sig_aggregate(c, n, len, t, d_ids.as<uint64_t>(), d_p1.as<uint8_t>(), d_pts.as<uint8_t>(),
                                    d_o1.as<uint8_t>(), d_out.as<uint8_t>(), st);
    });
    f.down(out_s2, d_out, n * sb);
    f.down(out_s1, d_o1, n * sb);
    return f.finish();
}

cc_status cc_verkey_aggregate_batch(cc_ctx* c, size_t n, size_t len, size_t t, size_t q, const uint64_t* ids,
                                    const uint8_t* X, const uint8_t* Y, uint8_t* outX, uint8_t* outY) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!ids || !X || !outX || (q && (!Y || !outY))))) return CC_ERR_DECODE;
    if (cc_status e = agg_checks(n, len, t)) return e;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    size_t ob = (size_t)oth_bytes(c->mode);
    int og = oth_group(c->mode);
    hipStream_t st = c->stream;
    DevBuf &d_ids = c->in_aux[0], &d_X = c->in_aux[1], &d_Y = c->in_aux[3], &d_oX = c->in_aux[2],
           &d_oY = c->in_aux[4];
    size_t ntask_y = n * q;
    size_t maxtask = ntask_y > n ? ntask_y : n;
    if (d_ids.ensure(n * len * 8) || d_X.ensure(n * len * ob) || d_Y.ensure(n * len * q * ob + 16) ||
        d_oX.ensure(n * ob) || d_oY.ensure(ntask_y * ob + 16) || c->lag.ensure(n * t * 32 + 32))
        return CC_ERR_HIP;
    cc_status s = agg_scratch(c, og, maxtask, t);
    if (s) return s;
    HostForm f(st);
    f.up(d_ids, ids, n * len * 8);
    f.up(d_X, X, n * len * ob);
    f.up(d_Y, Y, n * len * q * ob);
    f.launch([&]() -> cc_status {
        KCK(cck_lagrange(n, len, t, d_ids.as<uint64_t>(), c->lag.as<uint32_t>(), st));
        KCK(cck_msm_straus(og, n, t, d_X.as<uint8_t>(), len * ob, 0, ob, c->lag.as<uint32_t>(), 1,
                           c->agg_scratch.as<uint32_t>(), d_oX.as<uint8_t>(), st));
        if (q)
            KCK(cck_msm_straus(og, ntask_y, t, d_Y.as<uint8_t>(), len * q * ob, ob, q * ob, c->lag.as<uint32_t>(), q,
                               c->agg_scratch.as<uint32_t>(), d_oY.as<uint8_t>(), st));
        return CC_OK;
    });
    f.down(outX, d_oX, n * ob);
    f.down(outY, d_oY, ntask_y * ob);
    return f.finish();
}

// ---------------------------------------------------------------- issuer table (config 4)
cc_status cc_set_issuers(cc_ctx* c, size_t n_iss, size_t q, const uint64_t* ids, const uint8_t* X, const uint8_t* Y) {
    if (!c || !n_iss || !ids || !X || (q && !Y) || n_iss > (1u << 20) || q > 4096) return CC_ERR_DECODE;
    if (!c->peers.empty()) {
        for (cc_ctx* p : c->peers) {
            cc_status s = cc_set_issuers(p, n_iss, q, ids, X, Y);
            if (s) return s;
        }
        return CC_OK;
    }
    // no issuer table until every step below has succeeded (a failed call leaves CC_ERR_STATE behind,
    // never stale metadata over a rebuilt buffer)
    c->iss_n = 0;
    c->iss_q = 0;
    c->iss_ids_host.clear();
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent verify batches (cc_set_concurrency) use buffers rebuilt here
    const int og = oth_group(c->mode);
    const size_t ob = (size_t)oth_bytes(c->mode), aw = aff_words(og);
    // rows sorted by id; ids must be unique (they are the signers' Shamir x-coordinates)
    std::vector<size_t> ord(n_iss);
    for (size_t k = 0; k < n_iss; k++) ord[k] = k;
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return ids[a] < ids[b]; });
    for (size_t k = 1; k < n_iss; k++)
        if (ids[ord[k]] == ids[ord[k - 1]]) return CC_ERR_DECODE;
    const size_t nb = n_iss * (q + 1);
    std::vector<uint8_t> enc(nb * ob);
    std::vector<uint64_t> sid(n_iss);
    for (size_t r = 0; r < n_iss; r++) {
        const size_t k = ord[r];
        sid[r] = ids[k];
        memcpy(&enc[(r * (q + 1)) * ob], X + k * ob, ob);
        for (size_t j = 0; j < q; j++) memcpy(&enc[(r * (q + 1) + 1 + j) * ob], Y + (k * q + j) * ob, ob);
    }
    // the widest window whose tables fit the budget (16 GiB of the 288 GB HBM, at most half of what is
    // free; cc_set_table_bits forces a width): t x nwin additions per aggregated key, nwin = ceil(256 / w).
    c->iss_table.release();
    auto tbytes = [&](int w) { return nb * tab_words(og, w) * 4; };
    int wb = pick_table_bits(c->force_iss_bits, 16.0 * (double)(1ull << 30), tbytes);
    if (c->iss_ids.ensure(n_iss * 8) || c->iss_aff.ensure(nb * aw * 4) || c->iss_inf.ensure(nb * 4))
        return CC_ERR_HIP;
    wb = alloc_tables(wb, c->force_iss_bits != 0, tbytes, [&](int w) { return c->iss_table.ensure(tbytes(w)) == 0; });
    if (!wb) return CC_ERR_HIP;
    cc_status s = decode_points_host(c, og, nb, enc.data(), c->iss_aff.as<uint32_t>(), c->iss_inf.as<uint32_t>());
    if (s) return s;
    HIPCK(hipMemcpy(c->iss_ids.p, sid.data(), n_iss * 8, hipMemcpyHostToDevice));
    DevBuf pw;
    if (pw.ensure(nb * tab_nwin(wb) * (og == 1 ? 36 : 72) * 4)) return CC_ERR_HIP;
    KCK(cck_build_table(og, (int)nb, wb, c->iss_aff.as<uint32_t>(), c->iss_inf.as<uint32_t>(), pw.as<uint32_t>(),
                        c->iss_table.as<uint32_t>(), 1, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->iss_n = n_iss;
    c->iss_q = q;
    c->iss_wbits = wb;
    c->iss_ids_host = sid;
    return CC_OK;
}

cc_status cc_verkey_aggregate_ids_device(cc_ctx* c, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                         uint8_t* d_outX, uint8_t* d_outY, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_ids || !d_outX || (c->iss_q && !d_outY)))) return CC_ERR_DECODE;
    if (!c->iss_n) return CC_ERR_STATE;
    if (cc_status e = agg_checks(n, len, t)) return e;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    cc_status s = launch_vk_aggregate_ids(c, n, len, t, d_ids, d_outX, d_outY, st);
    if (s) return s;
    if (c->timing) collect_timing(c);
    return CC_OK;
}

// Signature::aggregate + Verkey::aggregate of the same credentials (same id lists): the Lagrange
// coefficients depend only on the ids (signature.rs:454-463 and 496-509 compute the same l_i), so one
// k_lagrange launch serves both MSMs.  Timing: (Lagrange, signature MSM, verkey MSM).
cc_status cc_aggregate_credential_batch_device(cc_ctx* c, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                               const uint8_t* d_s1, const uint8_t* d_s2, uint8_t* d_out_s1,
                                               uint8_t* d_out_s2, uint8_t* d_outX, uint8_t* d_outY, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_ids || !d_s1 || !d_s2 || !d_out_s1 || !d_out_s2 || !d_outX || (c->iss_q && !d_outY))))
        return CC_ERR_DECODE;
    if (!c->iss_n) return CC_ERR_STATE;
    if (cc_status e = agg_checks(n, len, t)) return e;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    const size_t sb = (size_t)sig_bytes(c->mode);
    const int sg = sig_group(c->mode);
    if (c->lag.ensure(n * t * 32 + 32)) return CC_ERR_HIP;
    cc_status s = agg_scratch(c, sg, n, t);
    if (s) return s;
    if (!c->dev_err.p) {
        if (c->dev_err.ensure(4)) return CC_ERR_HIP;
        HIPCK(hipMemsetAsync(c->dev_err.p, 0, 4, st));
    }
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
    // sigma_1 = sigs[0].sigma_1 (signature.rs:452): depends on neither MSM, so it goes first (behind the
    // Straus launch's one round of wave slots it waited milliseconds for a free slot)
    KCK(cck_copy_rows(n, sb, d_s1, len * sb, d_out_s1, st));
    KCK(cck_lagrange(n, len, t, d_ids, c->lag.as<uint32_t>(), st));
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    // the two MSMs share only the Lagrange coefficients: Signature::aggregate first on the caller's
    // stream (its launch is sized to one round of wave slots, cck_msm_straus), Verkey::aggregate on the
    // side stream behind it, filling the slots the Straus launch leaves and its tail
    hipStream_t side = c->side ? c->side : st;
    if (side != st) HIPCK(hipEventRecord(c->ev_fork, st));  // the coefficients are ready
    KCK(cck_msm_straus(sg, n, t, d_s2, len * sb, 0, sb, c->lag.as<uint32_t>(), 1, c->agg_scratch.as<uint32_t>(),
                       d_out_s2, st));
    if (side != st) HIPCK(hipStreamWaitEvent(side, c->ev_fork, 0));
    KCK(cck_vk_agg_fixed(oth_group(c->mode), n, len, t, (int)c->iss_q, d_ids, c->lag.as<uint32_t>(),
                         c->iss_ids.as<uint64_t>(), (int)c->iss_n, c->iss_table.as<uint32_t>(), c->iss_wbits,
                         c->iss_inf.as<uint32_t>(), d_outX, d_outY, c->dev_err.as<uint32_t>(), side));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    if (side != st) {
        HIPCK(hipEventRecord(c->ev_join, side));
        HIPCK(hipStreamWaitEvent(st, c->ev_join, 0));
    }
    if (c->timing) {
        (void)hipEventRecord(c->ev[3], st);  // phases: Lagrange, Signature::aggregate (sharing the GPU), the
        collect_timing(c);                   // rest of Verkey::aggregate after it
    }
    return CC_OK;
}

cc_status cc_verkey_aggregate_ids(cc_ctx* c, size_t n, size_t len, size_t t, const uint64_t* ids, uint8_t* outX,
                                  uint8_t* outY) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!ids || !outX || (c->iss_q && !outY)))) return CC_ERR_DECODE;
    if (!c->iss_n) return CC_ERR_STATE;
    if (cc_status e = agg_checks(n, len, t)) return e;
    if (!n) return CC_OK;
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < t; k++)
            if (!std::binary_search(c->iss_ids_host.begin(), c->iss_ids_host.end(), ids[i * len + k]))
                return CC_ERR_DECODE;  // id without an issuer verkey (the reference indexes a missing key)
    HIPCK(hipSetDevice(c->device));
    const size_t ob = (size_t)oth_bytes(c->mode), q = c->iss_q;
    hipStream_t st = c->stream;
    DevBuf &d_ids = c->in_aux[0], &d_oX = c->in_aux[2], &d_oY = c->in_aux[4];
    if (d_ids.ensure(n * len * 8) || d_oX.ensure(n * ob) || d_oY.ensure(n * q * ob + 16)) return CC_ERR_HIP;
    HostForm f(st);
    f.up(d_ids, ids, n * len * 8);
    f.launch([&] {
        return launch_vk_aggregate_ids(c, n, len, t, d_ids.as<uint64_t>(), d_oX.as<uint8_t>(), d_oY.as<uint8_t>(), st);
    });
    f.down(outX, d_oX, n * ob);
    f.down(outY, d_oY, n * q * ob);
    return f.finish();
}
