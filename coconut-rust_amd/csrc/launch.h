// The host launchers of the HIP kernels (cck_*): declared once, for the C ABI sources that call them and
// for the .hip files that define them.  C linkage admits no overloads, so a definition whose parameters
// differ from its declaration here does not compile (instead of linking and passing garbage).
// miller_lz.hip is compiled six ways and defines a different subset each time.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

extern "C" {
int cck_decode_points(int group, size_t n, const uint8_t* d_bytes, uint32_t* d_out, uint32_t* d_inf, hipStream_t st);
int cck_build_table(int group, int nbases, int wbits, const uint32_t* d_bases, const uint32_t* d_inf, uint32_t* d_pw,
                    uint32_t* d_table, int lazy_g2, hipStream_t st);
int cck_gtilde_lines(const uint32_t* d_gtilde_aff, uint32_t* d_lines, hipStream_t st);
int cck_flag_pair1(size_t n, uint32_t* d_flags, hipStream_t st);
int cck_lazy_form(size_t n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);
int cck_subgroup(int group, size_t n, const uint8_t* d_bytes, uint8_t* d_status, hipStream_t st);
int cck_hash_to_curve(int group, size_t n, const uint8_t* d_data, const uint64_t* d_offsets, uint8_t* d_out,
                      uint32_t* d_fail, hipStream_t st);
int cck_shake256_48(size_t n, const uint8_t* d_data, const uint64_t* d_offsets, uint8_t* d_out, hipStream_t st);
size_t cck_sigreq_proof_bytes(int group, int k);
int cck_vss_verify(size_t n, int t, const uint8_t* d_g, const uint8_t* d_h, const uint8_t* d_comms,
                   const uint32_t* d_set_of, const uint64_t* d_ids, const uint8_t* d_shares, uint32_t* d_scratch,
                   uint8_t* d_ok, hipStream_t st);
int cck_blind_assemble(int group, size_t n, int q, int k, const uint8_t* d_cts, const uint8_t* d_h,
                       const uint8_t* d_known, const uint8_t* d_x, const uint8_t* d_y, uint8_t* d_pts, uint32_t* d_sc,
                       hipStream_t st);
size_t cck_sigreq_scratch_words(int group, size_t n, int k);
int cck_sigreq_verify(int group, size_t n, int k, const uint8_t* d_g, const uint8_t* d_hvec, const uint8_t* d_comm,
                      const uint8_t* d_cts, const uint8_t* d_pk, const uint8_t* d_proof, const uint8_t* d_chal,
                      const uint8_t* d_hpts, uint32_t* d_scratch, uint8_t* d_ok, uint8_t* d_verdicts, hipStream_t st);
int cck_prep(int mode, size_t n, int q, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs,
             const uint32_t* d_Xaff, uint32_t Xinf, const uint32_t* d_table, int wbits, const uint32_t* d_binf_fixed,
             uint32_t* d_prep, uint32_t* d_flags, hipStream_t st);
int cck_prep_wide(int mode, size_t n, int q, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs,
                  const uint32_t* d_Xaff, uint32_t Xinf, const uint32_t* d_table, int wbits, const uint32_t* d_binf_fixed,
                  uint32_t* d_prep, uint32_t* d_flags, hipStream_t st);
size_t cck_prep_var_words(int mode, size_t n, size_t q);
int cck_prep_var(int mode, size_t n, int q, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_vkX,
                 const uint8_t* d_vkY, const uint8_t* d_msgs, uint32_t* d_scratch, uint32_t* d_prep,
                 uint32_t* d_flags, int wide, hipStream_t st);
int cck_miller_lz_g2(int twin, size_t n, size_t pstride, const uint32_t* d_prep, const uint32_t* d_flags,
                     const uint32_t* d_const, uint32_t* d_f, size_t fstride, size_t foff, uint32_t* d_qcheck,
                     hipStream_t st);
int cck_miller_lz_g1(int twin, size_t n, size_t pstride, const uint32_t* d_prep, const uint32_t* d_flags,
                     const uint32_t* d_const, uint32_t* d_f, size_t fstride, size_t foff, uint32_t* d_qcheck,
                     hipStream_t st);
int cck_miller4_lz_g2(size_t n, size_t pstride, const uint32_t* d_prep, const uint32_t* d_flags, uint32_t* d_f,
                      size_t fstride, size_t foff, uint32_t* d_qcheck, hipStream_t st);
int cck_miller4_lz_g1(size_t n, size_t pstride, const uint32_t* d_prep, const uint32_t* d_flags, uint32_t* d_f,
                      size_t fstride, size_t foff, uint32_t* d_qcheck, hipStream_t st);
size_t cck_fold_words(int mode, size_t n);
int cck_fold_pseudo();
int cck_fold_window(int mode, size_t n, uint32_t* d_work, uint32_t* d_partial, hipStream_t st);
int cck_fold(int mode, size_t n, const int8_t* d_dig, const uint32_t* d_pts, uint32_t* d_work, hipStream_t st);
int cck_fold_fixed(int mode, int q, const uint32_t* d_table, int wbits, const uint32_t* d_binf, uint32_t* d_pw,
                   uint8_t* d_finf, hipStream_t st);
int cck_miller_wide(size_t n, const uint32_t* d_prep, const uint32_t* d_flags, uint32_t* d_f, size_t fstride,
                    size_t foff, hipStream_t st);
int cck_f12_reduce_wide(size_t n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);
int cck_wide_pairs(int mode, size_t n, size_t ps, const uint32_t* d_prep, const uint32_t* d_flags,
                   const uint32_t* d_gaff, uint32_t* d_wprep, uint32_t* d_wflags, hipStream_t st);
int cck_fexp(size_t n, uint32_t* d_f, uint32_t* d_scratch, const uint32_t* d_flags, uint8_t* d_verdicts,
             uint8_t* d_gt, size_t wide_max, hipStream_t st);
int cck_lagrange(size_t n, size_t len, size_t t, const uint64_t* d_ids, uint32_t* d_l, hipStream_t st);
int cck_h_input_canon(int group, size_t n, size_t len, int kn, uint8_t* d_data, hipStream_t st);

size_t cck_straus_words(int group, size_t t);
int cck_msm_straus(int group, size_t ntask, size_t t, const uint8_t* d_pts, size_t pt_stride, size_t pt_jstride,
                   size_t pt_step, const uint32_t* d_l, size_t l_div, uint32_t* d_scratch, uint8_t* d_out,
                   hipStream_t st);
int cck_vk_agg_fixed(int group, size_t n, size_t len, size_t t, int q, const uint64_t* d_ids, const uint32_t* d_l,
                     const uint64_t* d_iss_ids, int n_iss, const uint32_t* d_table, int wbits, const uint32_t* d_binf,
                     uint8_t* d_outX, uint8_t* d_outY, uint32_t* d_err, hipStream_t st);
int cck_copy_rows(size_t n, size_t sb, const uint8_t* d_src, size_t pitch, uint8_t* d_dst, hipStream_t st);
int cck_fixed_mul(int group, size_t n, const uint8_t* d_ks, const uint32_t* d_table, uint32_t base_inf,
                  uint8_t* d_out, hipStream_t st);
int cck_prep_rlc(int mode, int part, size_t n, size_t ps, int q, uint64_t base_index, const uint32_t* d_key,
                 const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_msgs, const uint32_t* d_table, int wbits,
                 const uint32_t* d_binf, uint32_t* d_prep, uint32_t* d_flags, uint32_t* d_any, uint32_t* d_pts,
                 int8_t* d_dig, hipStream_t st);
int cck_rlc_reduce(size_t n, uint32_t* d_a, uint32_t* d_b, const uint32_t* d_any, uint32_t* d_partial,
                   hipStream_t st);
int cck_rlc_gather(int mode, size_t k, const uint32_t* d_parts, const uint32_t* d_pw, const uint8_t* d_finf,
                   uint32_t* d_fw, size_t fs, uint32_t* d_prep, uint32_t* d_flags2, uint32_t* d_flag, hipStream_t st);
// the segmented RLC partial and the per-partial finish (fold.hip, rlc.hip, miller_lz.hip with CC_MILLER_SEG)
size_t cck_fold_seg_words(int mode, size_t n, size_t seg);
int cck_fold_seg(int mode, size_t n, size_t seg, const int8_t* d_dig, const uint32_t* d_pts, uint32_t* d_work,
                 hipStream_t st);
int cck_fold_window_seg(int mode, size_t n, size_t seg, uint32_t* d_work, uint32_t* d_partials, hipStream_t st);
int cck_miller4_seg_lz_g2(size_t n, size_t pstride, const uint32_t* d_prep, const uint32_t* d_flags, uint32_t* d_f,
                          size_t fstride, size_t foff, uint32_t* d_qcheck, int qshift, hipStream_t st);
int cck_miller_twin_seg_lz_g2(size_t n, size_t pstride, const uint32_t* d_prep, const uint32_t* d_flags, uint32_t* d_f,
                              size_t fstride, size_t foff, uint32_t* d_qcheck, int qshift, hipStream_t st);
int cck_rlc_seg_flags(size_t n, int segsh, const uint32_t* d_flags, uint32_t* d_any, hipStream_t st);
int cck_rlc_seg_flags_pok(size_t n, int segsh, const uint32_t* d_flags, uint32_t* d_any, hipStream_t st);
int cck_rlc_reduce_seg(size_t n, size_t nseg, uint32_t* d_a, uint32_t* d_b, const uint32_t* d_any, uint32_t force,
                       uint32_t* d_partials, hipStream_t st);
int cck_rlc_gather_each(int mode, size_t k, const uint32_t* d_parts, const uint32_t* d_pw, const uint8_t* d_finf,
                        uint32_t* d_prep, uint32_t* d_flags2, uint32_t* d_flags, hipStream_t st);
int cck_rlc_each_products(size_t k, uint32_t* d_w, uint32_t* d_t, const uint32_t* d_parts, hipStream_t st);
int cck_prep_pok(int mode, size_t n, int q, int r, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_J,
                 const uint8_t* d_T, const uint8_t* d_resp, const uint8_t* d_chal, const uint8_t* d_rev_msgs,
                 const uint32_t* d_rev_idx, const uint32_t* d_Xaff, uint32_t Xinf, const uint32_t* d_table, int wbits,
                 const uint32_t* d_binf, uint32_t* d_prep, uint32_t* d_flags, uint32_t* d_jtab, hipStream_t st);
int cck_prep_pok_rlc(int mode, size_t n, size_t ps, int q, int r, uint64_t base_index, const uint32_t* d_key,
                     const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_resp, const uint8_t* d_chal,
                     const uint8_t* d_rev_msgs, const uint32_t* d_rev_idx, const uint32_t* d_table, int wbits,
                     const uint32_t* d_binf, uint32_t* d_prep, uint32_t* d_flags, uint32_t* d_any, uint32_t* d_jtab,
                     hipStream_t st);
int cck_prep_pok_wide(int mode, size_t n, int q, int r, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_J,
                 const uint8_t* d_T, const uint8_t* d_resp, const uint8_t* d_chal, const uint8_t* d_rev_msgs,
                 const uint32_t* d_rev_idx, const uint32_t* d_Xaff, uint32_t Xinf, const uint32_t* d_table, int wbits,
                 const uint32_t* d_binf, uint32_t* d_prep, uint32_t* d_flags, uint32_t* d_jtab, hipStream_t st);
size_t cck_prep_pok_var_words(int mode, size_t n, size_t q);
int cck_prep_pok_var(int mode, size_t n, int q, int r, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_J,
                     const uint8_t* d_T, const uint8_t* d_resp, const uint8_t* d_chal, const uint8_t* d_rev_msgs,
                     const uint32_t* d_rev_idx, const uint8_t* d_vkX, const uint8_t* d_vkY, const uint32_t* d_gaff,
                     uint32_t ginf, uint32_t* d_scratch, uint32_t* d_prep, uint32_t* d_flags, hipStream_t st);
size_t cck_sigma_prime_words(int mode, size_t n);
int cck_sigma_prime(int mode, size_t n, size_t rstride, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_rnd,
                    uint32_t* d_scratch, uint8_t* d_o1, uint8_t* d_o2, hipStream_t st);
int cck_pok_commit(int mode, size_t n, int q, int r, const uint8_t* d_msgs, const uint8_t* d_rnd,
                   const uint32_t* d_rev_idx, const uint32_t* d_table, int wbits, const uint32_t* d_binf, uint8_t* d_J,
                   uint8_t* d_T, hipStream_t st);
int cck_pok_responses(size_t n, int q, int r, const uint8_t* d_msgs, const uint8_t* d_rnd, const uint8_t* d_chal,
                      const uint32_t* d_rev_idx, uint8_t* d_out, hipStream_t st);
int cck_unblind_assemble(int group, size_t n, const uint8_t* d_c1, const uint8_t* d_c2, const uint8_t* d_sk,
                         uint8_t* d_pts, uint32_t* d_sc, hipStream_t st);
size_t cck_rq_table_words(int group, size_t n);
size_t cck_rq_digit_bytes(size_t n, int k);
int cck_rq_fixed(int group, size_t n, int q, int k, int init, const uint8_t* d_msgs, const uint8_t* d_rnd,
                 const uint32_t* d_table, int wbits, const uint32_t* d_binf, uint8_t* d_long, uint8_t* d_out,
                 hipStream_t st);
int cck_rq_two_base(int group, size_t n, int q, int k, int init, const uint8_t* d_pk, const uint8_t* d_h,
                    const uint8_t* d_msgs, const uint8_t* d_rnd, uint32_t* d_tab, int8_t* d_digs, uint8_t* d_out,
                    hipStream_t st);
int cck_rq_h_rows(int group, size_t n, int q, int k, const uint8_t* d_commitment, const uint8_t* d_msgs,
                  uint8_t* d_data, uint64_t* d_offsets, hipStream_t st);
size_t cck_iv_table_words(int group, size_t n, int k);
size_t cck_iv_cdig_bytes(size_t n);
size_t cck_iv_dig_bytes(size_t n, int k);
size_t cck_iv_ok_bytes(size_t n, int k);
int cck_iv_checks(int group, size_t n, int q, int k, const uint8_t* d_comm, const uint8_t* d_cts, const uint8_t* d_pk,
                  const uint8_t* d_proof, const uint8_t* d_chal, const uint8_t* d_h, const uint32_t* d_table,
                  int wbits, const uint32_t* d_binf, uint32_t* d_tab, int8_t* d_cdig, int8_t* d_digs, uint8_t* d_ok,
                  hipStream_t st);
int cck_sigreq_combine(int group, size_t n, int k, const uint8_t* d_proof, const uint8_t* d_ok, uint8_t* d_verdicts,
                       hipStream_t st);
int cck_rq_responses(int group, size_t n, int q, int k, const uint8_t* d_msgs, const uint8_t* d_rnd,
                     const uint8_t* d_blind, const uint8_t* d_sk, const uint8_t* d_chal, uint8_t* d_proofs,
                     hipStream_t st);
int cck_kg_eval(size_t m, int q, int t, int total, const uint8_t* d_cf, const uint8_t* d_ct, uint8_t* d_x, uint8_t* d_y,
                uint8_t* d_xt, uint8_t* d_yt, hipStream_t st);
int cck_kg_commit(size_t n, const uint8_t* d_cf, const uint8_t* d_ct, const uint32_t* d_table, int wbits,
                  const uint32_t* d_binf, uint8_t* d_out, hipStream_t st);
int cck_kg_derive(int group, size_t nrow, int q, const uint8_t* d_x, const uint8_t* d_y, const uint32_t* d_table,
                  int wbits, const uint32_t* d_binf, uint8_t* d_X, uint8_t* d_Y, hipStream_t st);
int cck_kg_sum(int g1, size_t m, size_t inner, int d, const uint8_t* d_in, uint8_t* d_out, hipStream_t st);
// Pedersen VSS verify_share over commitment sets (vss.hip).  How a launch finds its rows: the CSR form
// (set_begin non-NULL: set j holds rows [set_begin[j], set_begin[j + 1]) of ids / shares), or the keygen
// outputs in place (set_begin NULL: set j = keygen (q + 1) + p holds signers 1 .. total, rows
// [j total, (j + 1) total), shares at keygen.hip's kg_share_off in x / y and xt / yt).  Device pointers.
struct cck_vss_rows {
    const uint64_t* set_begin;
    const uint64_t* ids;
    const uint8_t* shares;
    const uint8_t *x, *y, *xt, *yt;
    uint32_t q, total;
};
size_t cck_vss_prep_words(size_t npts);
size_t cck_vss_msm_words(size_t t);
int cck_vss_prep(size_t npts, int t, const uint8_t* d_comms, const uint8_t* d_gh, uint32_t* d_prep, uint32_t* d_set_flag,
                 uint32_t* d_gh_flag, uint8_t* d_gh_neg, hipStream_t st);
int cck_vss_exact(size_t nrow, int t, const cck_vss_rows* rows, const uint32_t* d_sel_set, const uint64_t* d_sel_off,
                  size_t nsel, const uint32_t* d_prep, const uint32_t* d_table, int wbits, const uint32_t* d_binf,
                  uint8_t* d_verdicts, hipStream_t st);
int cck_vss_scalars(size_t n_sets, int t, const cck_vss_rows* rows, const uint32_t* d_key, uint32_t* d_A, uint32_t* d_UU,
                    hipStream_t st);
int cck_vss_msm(size_t j0, size_t cnt, int t, const uint8_t* d_comms, const uint32_t* d_A, const uint32_t* d_UU,
                const uint32_t* d_table, int wbits, const uint32_t* d_binf, const uint32_t* d_set_flag,
                const uint32_t* d_gh_flag, uint32_t* d_scratch, uint8_t* d_status, hipStream_t st);
int cck_vss_status(size_t n_sets, const uint32_t* d_set_flag, const uint32_t* d_gh_flag, uint8_t* d_status,
                   hipStream_t st);
int cck_vss_fill(size_t n, size_t n_sets, const cck_vss_rows* rows, const uint8_t* d_status, uint8_t* d_verdicts,
                 hipStream_t st);
int cck_vss_gather(size_t nrow, const cck_vss_rows* rows, const uint32_t* d_sel_set, const uint64_t* d_sel_off,
                   size_t nsel, uint32_t* d_set_of, uint64_t* d_ids, uint8_t* d_shares, uint64_t* d_row_of,
                   hipStream_t st);
int cck_vss_scatter(size_t nrow, const uint64_t* d_row_of, const uint8_t* d_ok, uint8_t* d_verdicts, hipStream_t st);
int cck_rlc_partial_words();
int cck_fexp_q(size_t n, const uint32_t* d_f, const uint32_t* d_flags, uint8_t* d_verdicts, uint8_t* d_gt,
               hipStream_t st);
}
