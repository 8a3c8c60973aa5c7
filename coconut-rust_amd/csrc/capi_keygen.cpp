// C ABI, keygen: the keygen params, Shamir / Pedersen VSS dealing and the DVSS combine (ctx.h).
#include "ctx.h"

// ---------------------------------------------------------------- keygen: dealing and the DVSS combine (keygen.hip)
// default HBM budget of the keygen tables (at most half of what is free): at 16 bits 0.10 / 0.20 GB for a
// G1 / G2 g~ and 0.20 GB for [g, h]
constexpr double kKgTableBudget = 4.0 * (double)(1ull << 30);

cc_status cc_set_keygen_params(cc_ctx* c, const uint8_t* g_tilde, const uint8_t* vss_g, const uint8_t* vss_h,
                               int table_bits) {
    c = primary(c);  // a device set forwards to its first device
    if (!c) return CC_ERR_DECODE;
    // no keygen params until every step below has succeeded: any failed call, a refused argument included,
    // leaves the context without them
    c->have_kg = false;
    c->kg_have_gh = false;
    if (!g_tilde || (vss_g == nullptr) != (vss_h == nullptr) || (table_bits != 0 && (table_bits < 8 || table_bits > 16)))
        return CC_ERR_DECODE;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches before the tables are rebuilt
    HIPCK(hipStreamSynchronize(c->stream));  // an asynchronous *_device call may still read the old tables
    const int og = oth_group(c->mode);
    const bool gh = vss_g != nullptr;
    auto tbytes = [&](int w) { return (tab_words(og, w) + (gh ? 2 * tab_words(1, w) : 0)) * 4; };
    c->kg_gt_table.release();
    c->kg_gh_table.release();
    int wb = pick_table_bits(table_bits, kKgTableBudget, tbytes);
    if (c->kg_gt_aff.ensure(aff_words(og) * 4) || c->kg_gt_inf.ensure(4) || c->kg_gh_aff.ensure(2 * aff_words(1) * 4) ||
        c->kg_gh_inf.ensure(2 * 4))
        return CC_ERR_HIP;
    wb = alloc_tables(wb, table_bits != 0, tbytes, [&](int w) {
        if (c->kg_gt_table.ensure(tab_words(og, w) * 4) == 0 && (!gh || c->kg_gh_table.ensure(2 * tab_words(1, w) * 4) == 0))
            return true;
        c->kg_gt_table.release();  // neither without the other
        c->kg_gh_table.release();
        return false;
    });
    if (!wb) return CC_ERR_HIP;
    cc_status s = decode_points_host(c, og, 1, g_tilde, c->kg_gt_aff.as<uint32_t>(), c->kg_gt_inf.as<uint32_t>());
    if (s) return s;
    DevBuf pw;
    if (pw.ensure(2 * tab_nwin(wb) * 72 * 4)) return CC_ERR_HIP;
    // lazy form: the sums read the tables through ft_add_lz / pl::ft_add_g2_lz
    KCK(cck_build_table(og, 1, wb, c->kg_gt_aff.as<uint32_t>(), c->kg_gt_inf.as<uint32_t>(), pw.as<uint32_t>(),
                        c->kg_gt_table.as<uint32_t>(), 1, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (gh) {
        uint8_t enc[2 * 97];
        memcpy(enc, vss_g, 97);
        memcpy(enc + 97, vss_h, 97);
        s = decode_points_host(c, 1, 2, enc, c->kg_gh_aff.as<uint32_t>(), c->kg_gh_inf.as<uint32_t>());
        if (s) return s;
        if (c->kg_gh_enc.ensure(2 * 97)) return CC_ERR_HIP;
        KCK(HipMem::h2d(c->kg_gh_enc.p, enc, 2 * 97, c->stream));  // synchronised below
        KCK(cck_build_table(1, 2, wb, c->kg_gh_aff.as<uint32_t>(), c->kg_gh_inf.as<uint32_t>(), pw.as<uint32_t>(),
                            c->kg_gh_table.as<uint32_t>(), 1, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    }
    c->kg_wbits = wb;
    c->kg_have_gh = gh;
    c->have_kg = true;
    return CC_OK;
}

// the checks after the NULL checks, in the header's order; md: keygens the buffers hold (combine: m x d)
static cc_status kg_checks(const cc_ctx* c, bool pedersen, size_t m, size_t d, size_t q, size_t t, size_t total) {
    if (!c->have_kg || (pedersen && !c->kg_have_gh)) return CC_ERR_STATE;
    if (t == 0 || t > total) return CC_ERR_THRESHOLD;
    if (d == 0 || total > kMaxIds || q > kMaxQ || m > kMaxBatch || d > kMaxBatch) return CC_ERR_DECODE;
    const size_t md = m * d;  // < 2^53
    if (md > kMaxBatch) return CC_ERR_DECODE;
    // md <= 2^26, total <= 2^16, q + 1 < 2^13: the products stay below 2^55
    if (md * total * (q + 1) > kMaxBatch || md * (q + 1) * t > kMaxBatch) return CC_ERR_DECODE;
    return CC_OK;
}

static cc_status launch_kg_deal(cc_ctx* c, size_t m, size_t q, size_t t, size_t total, const uint8_t* d_cf,
                                const uint8_t* d_ct, uint8_t* d_x, uint8_t* d_y, uint8_t* d_xt, uint8_t* d_yt,
                                uint8_t* d_comm, uint8_t* d_X, uint8_t* d_Y, hipStream_t st) {
    KCK(cck_kg_eval(m, (int)q, (int)t, (int)total, d_cf, d_ct, d_x, d_y, d_xt, d_yt, st));
    if (d_ct)
        KCK(cck_kg_commit(m * (q + 1) * t, d_cf, d_ct, c->kg_gh_table.as<uint32_t>(), c->kg_wbits,
                          c->kg_gh_inf.as<uint32_t>(), d_comm, st));
    KCK(cck_kg_derive(oth_group(c->mode), m * total, (int)q, d_x, d_y, c->kg_gt_table.as<uint32_t>(), c->kg_wbits,
                      c->kg_gt_inf.as<uint32_t>(), d_X, d_Y, st));
    return CC_OK;
}

// NULL checks of the deal: the buffers the call would read or write with m > 0
static bool kg_deal_null(size_t m, size_t q, const void* cf, const void* ct, const void* x, const void* y,
                         const void* xt, const void* yt, const void* comm, const void* X, const void* Y) {
    if (!m) return false;
    if (!cf || !x || !X || (q && (!y || !Y))) return true;
    return ct && (!xt || !comm || (q && !yt));
}

cc_status cc_keygen_deal_batch_device(cc_ctx* c, size_t m, size_t q, size_t t, size_t total, const uint8_t* d_coeffs,
                                      const uint8_t* d_coeffs_t, uint8_t* d_out_x, uint8_t* d_out_y,
                                      uint8_t* d_out_xt, uint8_t* d_out_yt, uint8_t* d_out_comm, uint8_t* d_out_X,
                                      uint8_t* d_out_Y, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || kg_deal_null(m, q, d_coeffs, d_coeffs_t, d_out_x, d_out_y, d_out_xt, d_out_yt, d_out_comm, d_out_X,
                           d_out_Y))
        return CC_ERR_DECODE;
    cc_status s = kg_checks(c, d_coeffs_t != nullptr, m, 1, q, t, total);
    if (s) return s;
    if (!m) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    return launch_kg_deal(c, m, q, t, total, d_coeffs, d_coeffs_t, d_out_x, d_out_y, d_out_xt, d_out_yt, d_out_comm,
                          d_out_X, d_out_Y, st);
}

cc_status cc_keygen_deal_batch(cc_ctx* c, size_t m, size_t q, size_t t, size_t total, const uint8_t* coeffs,
                               const uint8_t* coeffs_t, uint8_t* out_x, uint8_t* out_y, uint8_t* out_xt,
                               uint8_t* out_yt, uint8_t* out_comm, uint8_t* out_X, uint8_t* out_Y) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || kg_deal_null(m, q, coeffs, coeffs_t, out_x, out_y, out_xt, out_yt, out_comm, out_X, out_Y))
        return CC_ERR_DECODE;
    const bool ped = coeffs_t != nullptr;
    cc_status s = kg_checks(c, ped, m, 1, q, t, total);
    if (s) return s;
    if (!m) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t ob = (size_t)oth_bytes(c->mode);
    const size_t cb = m * (q + 1) * t * 48, xb = m * total * 48, yb = xb * q;
    const size_t mb = m * (q + 1) * t * 97, Xb = m * total * ob, Yb = Xb * q;
    hipStream_t st = c->stream;
    DevBuf* B = c->kg_io;  // coeffs, coeffs_t, x, y, xt, yt, comm, X, Y
    if (B[0].ensure(cb) || B[2].ensure(xb) || B[3].ensure(yb + 16) || B[7].ensure(Xb) || B[8].ensure(Yb + 16))
        return CC_ERR_HIP;
    if (ped && (B[1].ensure(cb) || B[4].ensure(xb) || B[5].ensure(yb + 16) || B[6].ensure(mb))) return CC_ERR_HIP;
    const size_t pxb = ped ? xb : 0, pyb = ped ? yb : 0;  // the Pedersen buffers' sizes: nothing without them
    HostForm f(st);
    f.up_secret(B[0], coeffs, cb);
    f.up_secret(B[1], coeffs_t, ped ? cb : 0);
    f.launch([&] {
        return launch_kg_deal(c, m, q, t, total, B[0].as<uint8_t>(), ped ? B[1].as<uint8_t>() : nullptr,
                              B[2].as<uint8_t>(), B[3].as<uint8_t>(), B[4].as<uint8_t>(), B[5].as<uint8_t>(),
                              B[6].as<uint8_t>(), B[7].as<uint8_t>(), B[8].as<uint8_t>(), st);
    });
    f.down_secret(out_x, B[2], xb);
    f.down(out_X, B[7], Xb);
    f.down_secret(out_y, B[3], yb);
    f.down(out_Y, B[8], Yb);
    f.down_secret(out_xt, B[4], pxb);
    f.down_secret(out_yt, B[5], pyb);
    f.down(out_comm, B[6], ped ? mb : 0);
    // zeroes the device copies of the coefficients and of the shares (the kernels keep the window digits in
    // registers: there is no digit scratch)
    return f.finish();
}

static cc_status launch_kg_combine(cc_ctx* c, size_t m, size_t d, size_t q, size_t t, size_t total, bool ped,
                                   const uint8_t* d_x, const uint8_t* d_y, const uint8_t* d_xt, const uint8_t* d_yt,
                                   const uint8_t* d_comm, uint8_t* d_ox, uint8_t* d_oy, uint8_t* d_oxt, uint8_t* d_oyt,
                                   uint8_t* d_ocomm, uint8_t* d_oX, uint8_t* d_oY, hipStream_t st) {
    KCK(cck_kg_sum(0, m, total, (int)d, d_x, d_ox, st));
    if (q) KCK(cck_kg_sum(0, m, total * q, (int)d, d_y, d_oy, st));
    if (ped) {
        KCK(cck_kg_sum(0, m, total, (int)d, d_xt, d_oxt, st));
        if (q) KCK(cck_kg_sum(0, m, total * q, (int)d, d_yt, d_oyt, st));
        KCK(cck_kg_sum(1, m, (q + 1) * t, (int)d, d_comm, d_ocomm, st));
    }
    KCK(cck_kg_derive(oth_group(c->mode), m * total, (int)q, d_ox, d_oy, c->kg_gt_table.as<uint32_t>(), c->kg_wbits,
                      c->kg_gt_inf.as<uint32_t>(), d_oX, d_oY, st));
    return CC_OK;
}

// NULL checks of the combine; ped: any of the Pedersen buffers given, then all of them are needed
static bool kg_combine_null(size_t m, size_t q, bool ped, const void* x, const void* y, const void* xt, const void* yt,
                            const void* comm, const void* ox, const void* oy, const void* oxt, const void* oyt,
                            const void* ocomm, const void* oX, const void* oY) {
    if (!m) return false;
    if (!x || !ox || !oX || (q && (!y || !oy || !oY))) return true;
    return ped && (!xt || !comm || !oxt || !ocomm || (q && (!yt || !oyt)));
}

cc_status cc_keygen_combine_batch_device(cc_ctx* c, size_t m, size_t d, size_t q, size_t t, size_t total,
                                         const uint8_t* d_x, const uint8_t* d_y, const uint8_t* d_xt,
                                         const uint8_t* d_yt, const uint8_t* d_comm, uint8_t* d_out_x,
                                         uint8_t* d_out_y, uint8_t* d_out_xt, uint8_t* d_out_yt, uint8_t* d_out_comm,
                                         uint8_t* d_out_X, uint8_t* d_out_Y, void* stream) {
    c = primary(c);  // a device set forwards to its first device
    const bool ped = d_xt || d_yt || d_comm || d_out_xt || d_out_yt || d_out_comm;
    if (!c || kg_combine_null(m, q, ped, d_x, d_y, d_xt, d_yt, d_comm, d_out_x, d_out_y, d_out_xt, d_out_yt, d_out_comm,
                              d_out_X, d_out_Y))
        return CC_ERR_DECODE;
    cc_status s = kg_checks(c, ped, m, d, q, t, total);
    if (s) return s;
    if (!m) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    StreamOrder order(c, st);
    return launch_kg_combine(c, m, d, q, t, total, ped, d_x, d_y, d_xt, d_yt, d_comm, d_out_x, d_out_y, d_out_xt,
                             d_out_yt, d_out_comm, d_out_X, d_out_Y, st);
}

cc_status cc_keygen_combine_batch(cc_ctx* c, size_t m, size_t d, size_t q, size_t t, size_t total, const uint8_t* x,
                                  const uint8_t* y, const uint8_t* xt, const uint8_t* yt, const uint8_t* comm,
                                  uint8_t* out_x, uint8_t* out_y, uint8_t* out_xt, uint8_t* out_yt, uint8_t* out_comm,
                                  uint8_t* out_X, uint8_t* out_Y) {
    c = primary(c);  // a device set forwards to its first device
    const bool ped = xt || yt || comm || out_xt || out_yt || out_comm;
    if (!c || kg_combine_null(m, q, ped, x, y, xt, yt, comm, out_x, out_y, out_xt, out_yt, out_comm, out_X, out_Y))
        return CC_ERR_DECODE;
    cc_status s = kg_checks(c, ped, m, d, q, t, total);
    if (s) return s;
    if (!m) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);  // concurrent device batches (cc_set_concurrency) before the workspaces are resized
    const size_t ob = (size_t)oth_bytes(c->mode);
    const size_t xb = m * total * 48, yb = xb * q, mb = m * (q + 1) * t * 97, Xb = m * total * ob, Yb = Xb * q;
    hipStream_t st = c->stream;
    DevBuf* B = c->kg_io;  // in: x, y, xt, yt, comm (d times the out sizes); out: x, y, xt, yt, comm, X, Y
    if (B[0].ensure(d * xb) || B[1].ensure(d * yb + 16) || B[5].ensure(xb) || B[6].ensure(yb + 16) ||
        B[10].ensure(Xb) || B[11].ensure(Yb + 16))
        return CC_ERR_HIP;
    if (ped && (B[2].ensure(d * xb) || B[3].ensure(d * yb + 16) || B[4].ensure(d * mb) || B[7].ensure(xb) ||
                B[8].ensure(yb + 16) || B[9].ensure(mb)))
        return CC_ERR_HIP;
    const size_t pxb = ped ? xb : 0, pyb = ped ? yb : 0;  // the Pedersen buffers' sizes: nothing without them
    HostForm f(st);
    f.up_secret(B[0], x, d * xb);
    f.up_secret(B[1], y, d * yb);
    f.up_secret(B[2], xt, d * pxb);
    f.up_secret(B[3], yt, d * pyb);
    f.up(B[4], comm, ped ? d * mb : 0);
    f.launch([&] {
        return launch_kg_combine(c, m, d, q, t, total, ped, B[0].as<uint8_t>(), B[1].as<uint8_t>(), B[2].as<uint8_t>(),
                                 B[3].as<uint8_t>(), B[4].as<uint8_t>(), B[5].as<uint8_t>(), B[6].as<uint8_t>(),
                                 B[7].as<uint8_t>(), B[8].as<uint8_t>(), B[9].as<uint8_t>(), B[10].as<uint8_t>(),
                                 B[11].as<uint8_t>(), st);
    });
    f.down_secret(out_x, B[5], xb);
    f.down(out_X, B[10], Xb);
    f.down_secret(out_y, B[6], yb);
    f.down(out_Y, B[11], Yb);
    f.down_secret(out_xt, B[7], pxb);
    f.down_secret(out_yt, B[8], pyb);
    f.down(out_comm, B[9], ped ? mb : 0);
    return f.finish();  // zeroes the device copies of the dealers' shares and of the combined shares
}
