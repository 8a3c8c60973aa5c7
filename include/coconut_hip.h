/* coconut_hip.h — C ABI of the MI355X batch-verification engine for Coconut credentials.
 *
 * Drop-in boundary for the reference's verifier hot path (3for/coconut-rust, read-only at
 * /root/reference).  The reference has no FFI of its own; these entry points are what its Rust
 * API would bind through `extern "C"` (binding shown in INTEGRATION.md):
 *
 *   cc_verify_batch / cc_verify_batch_device / cc_verify_batch_pervk_device
 *        replaces  Signature::verify              src/signature.rs:473-478
 *                  (-> ps_sig Signature::verify [EXT], via transforms signature.rs:83-104)
 *   cc_signature_aggregate_batch
 *        replaces  Signature::aggregate           src/signature.rs:448-470
 *   cc_verkey_aggregate_batch
 *        replaces  Verkey::aggregate              src/signature.rs:483-526
 *   cc_pok_verify_batch / cc_pok_verify_batch_pervk(_device)
 *        replaces  ps_sig PoKOfSignatureProof::verify [EXT], called at src/pok_sig.rs:103-105
 *   cc_pok_init_batch / cc_pok_gen_proof_batch
 *        replaces  ps_sig PoKOfSignature::init / gen_proof [EXT], called at src/pok_sig.rs:80-100
 *   cc_unblind_batch
 *        replaces  BlindSignature::unblind        src/signature.rs:436-443
 *   cc_sigreq_new_batch / cc_sigreq_pok_init_batch / cc_sigreq_pok_gen_proof_batch
 *        replaces  SignatureRequest::new, SignatureRequestPoK::init / gen_proof
 *                                                 src/signature.rs:124-192, 216-320
 *   cc_keygen_deal_batch / cc_keygen_combine_batch
 *        replaces  trusted_party_SSS_keygen, trusted_party_PVSS_keygen, keygen_from_shares and the
 *                  decentralized keygen's final sums  src/keygen.rs:17-122, 124-205
 *   cc_set_params / cc_set_verkey
 *        the Params (src/signature.rs:13-17, only g_tilde is read by verify) and Verkey
 *        (src/signature.rs:46-49) a batch is checked against
 *
 * Encodings are amcl_wrapper's `to_bytes`:
 *   Fr 48 B big-endian | G1 97 B = 0x04||x||y | G2 192 B = x.a||x.b||y.a||y.b | GT 576 B (AMCL FP12)
 * Group assignment (reference src/lib.rs:3-4,12-13): CC_SIG_G2 = the reference default build
 * (sigma, g, h in G2; X~, Y~, g~ in G1), CC_SIG_G1 = the other feature.
 *
 * All host pointers are caller-owned, read during the call and never retained.  A context owns
 * one HIP device, one stream and the device tables; use one context per calling thread.
 * A context made by cc_ctx_create_multi spans a device set (one single-device context and one RCCL
 * communicator per GPU, one host thread per GPU during a call): cc_set_params / cc_set_verkey apply
 * to every device and cc_verify_batch shards the batch by credential over the set (RLC mode: one
 * ncclAllGather of 3,716-byte partials over xGMI); the other entry points run on the
 * set's first device.
 * Streams: the *_device entry points take a caller stream; the library orders it against the
 * context's own stream (which the host entry points use) with events at entry and exit, so calls on
 * any mix of streams see the context's workspaces in program order.
 * Errors mirror the reference's failure modes (src/errors.rs:6-24): where the reference panics
 * (assert!/unwrap) the C ABI returns a code instead.
 * Empty batches: every batch entry point checks its context state and lengths first (CC_ERR_STATE,
 * CC_ERR_LEN, CC_ERR_BASES_EXPS, CC_ERR_THRESHOLD), then returns CC_OK for n = 0 without reading,
 * writing or launching anything; its buffer pointers may then be NULL (tests/test_gpu_empty.py).
 * Ceilings: n <= CC_MAX_BATCH credentials / proofs / points per call, an aggregation's ids per
 * credential (len) <= CC_MAX_IDS, q <= CC_MAX_Q messages, an RLC finish's gathered partials <=
 * CC_MAX_PARTS; a larger count is CC_ERR_DECODE before anything is read, allocated or launched (the
 * byte counts the library derives from them then never overflow).
 */
#ifndef COCONUT_HIP_H
#define COCONUT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CC_MAX_BATCH ((size_t)1 << 26)
#define CC_MAX_IDS ((size_t)1 << 16)
#define CC_MAX_Q ((size_t)4096)
#define CC_MAX_PARTS ((size_t)1 << 16)

typedef enum {
    CC_OK = 0,
    CC_ERR_LEN = -1,          /* CoconutErrorKind::UnsupportedNoOfMessages (verkey q != msgs)   */
    CC_ERR_BASES_EXPS = -2,   /* CoconutErrorKind::UnequalNoOfBasesExponents (PoK responses)    */
    CC_ERR_THRESHOLD = -3,    /* len < threshold: reference assert! panics (signature.rs:449,484) */
    CC_ERR_DECODE = -4,       /* malformed buffer sizes / missing params                           */
    CC_ERR_HIP = -5,          /* HIP runtime failure                                               */
    CC_ERR_RCCL = -6,         /* collective failure (RLC gather)                                   */
    CC_ERR_STATE = -7         /* call order: params / verkey not set                               */
} cc_status;

typedef enum { CC_SIG_G2 = 0, CC_SIG_G1 = 1 } cc_group_mode;

typedef struct cc_ctx cc_ctx;

const char* cc_status_str(int status);
const char* cc_version(void);

cc_status cc_ctx_create(int device, cc_group_mode mode, cc_ctx** out);
/* Device set: bit d of device_mask selects GPU d (SURVEY.md §8b `cc_ctx_create(device_mask, ...)`);
 * CC_ERR_RCCL if the communicators cannot be created. */
cc_status cc_ctx_create_multi(uint64_t device_mask, cc_group_mode mode, cc_ctx** out);
cc_status cc_ctx_num_devices(const cc_ctx* ctx, int* ndev);
cc_status cc_ctx_destroy(cc_ctx* ctx);
cc_status cc_ctx_mode(const cc_ctx* ctx, int* mode_out);

/* Params: only g_tilde (OtherGroup encoding) is used on the verify path.  The same g_tilde again is a
 * no-op.  A new g_tilde under a bound verkey keeps the verkey and rebuilds everything derived from both
 * (g~'s slot of the verkey block, the fixed-base tables and the RLC window points at the width they had or
 * the one cc_set_table_bits now asks for, the subgroup status the RLC depends on) before the call
 * returns, after waiting for the concurrency slots' batches; should that rebuild fail the context is left
 * WITHOUT a verkey, as after a failed cc_set_verkey.
 * A g_tilde that does not decode (the identity's encoding, a bad prefix, a point off the curve) is the
 * identity, as in the reference: every pairing with it is 1, so Signature::verify and the pairing half of
 * PoKOfSignatureProof::verify reduce to e(sigma_1, pr) = 1, the provers' J and T lose their g~ term, and
 * the RLC never accepts on its own (its verdicts come from the per-credential path).  Coordinates >= p
 * are reduced; a point on the curve outside the subgroup is paired as it is. */
cc_status cc_set_params(cc_ctx* ctx, const uint8_t* g_tilde);

/* Shared verkey (X~, Y~[q]) for cc_verify_batch with vk == NULL: builds fixed-base tables on the
 * device (one-time cost, reported separately from batch throughput): the widest of 22 / 20 / 18 / 16 /
 * 14 / 12 / 10-bit windows whose q + 2 bases' tables fit 4 GiB and 40 % of the free HBM, else 8-bit
 * windows (cc_set_table_bits forces a width).  The same verkey again (bytes and width unchanged) is a
 * no-op.  On any failure the context is left WITHOUT a verkey (verify / RLC / PoK calls then return
 * CC_ERR_STATE). */
cc_status cc_set_verkey(cc_ctx* ctx, const uint8_t* X, const uint8_t* Y, size_t q);

/* Window widths of the fixed-base tables built by later cc_set_verkey / cc_set_issuers calls:
 * verkey_bits 0 (chosen by memory) or 8..22; issuer_bits 0 (chosen by memory) or 8..16.  A forced
 * width that does not fit HBM makes the building call fail.  cc_table_bits reports the widths of the
 * current tables (0: none built). */
cc_status cc_set_table_bits(cc_ctx* ctx, int verkey_bits, int issuer_bits);
cc_status cc_table_bits(const cc_ctx* ctx, int* verkey_bits, int* issuer_bits);

/* Batch Signature::verify.
 *   sigma1, sigma2 : n x SignatureGroup encodings
 *   msgs           : n x q x 48 B
 *   vk_X, vk_Y     : NULL => the shared verkey from cc_set_verkey; else n x OtherGroup and
 *                    n x q x OtherGroup (one verkey per credential)
 *   verdicts       : n bytes, 1 = verify() returned true
 *   gt_or_null     : n x 576 B, e(.,.)*e(.,.) as amcl_wrapper GT::to_bytes, or NULL
 *   rlc            : 0 = per-credential; 1 = random-linear-combination batch (all-or-fallback)
 * Returns CC_ERR_LEN if q differs from the shared verkey's q (the reference panics there).
 * Batch size picks the kernels, not the results: a batch of up to 4,096 credentials runs latency-bound
 * (one wave per Miller pair; up to 2,048 also one per final exponentiation and per shared-verkey prep,
 * up to 1,024 one per per-credential-verkey or PoK prep), a larger one throughput-bound (one lane pair per credential); verdicts and GT bytes are the
 * same either way. */
cc_status cc_verify_batch(cc_ctx* ctx, size_t n, size_t q, const uint8_t* sigma1, const uint8_t* sigma2,
                          const uint8_t* msgs, const uint8_t* vk_X, const uint8_t* vk_Y, uint8_t* verdicts,
                          uint8_t* gt_or_null, int rlc);

/* Same, with every buffer already in device memory (HBM-resident batch; the timed bench path).
 * Shared verkey only.  `stream` is a hipStream_t or NULL for the context's stream.  The call is
 * asynchronous with respect to the host; synchronise the stream before reading verdicts. */
cc_status cc_verify_batch_device(cc_ctx* ctx, size_t n, size_t q, const uint8_t* d_sigma1, const uint8_t* d_sigma2,
                                 const uint8_t* d_msgs, uint8_t* d_verdicts, uint8_t* d_gt_or_null, void* stream);

/* Per-credential verkeys with every buffer in device memory: Signature::verify(msgs, vk_i, params) for
 * each credential i with ITS OWN verkey (src/signature.rs:473-478 takes the verkey per call;
 * ps_sig's var-time MSM over [X~, Y~_1..q]): d_vk_X n x OtherGroup, d_vk_Y n x q x OtherGroup, the
 * rest as cc_verify_batch_device.  Needs only cc_set_params (g~); q <= 4096.  Asynchronous on
 * `stream` (NULL: the context stream). */
cc_status cc_verify_batch_pervk_device(cc_ctx* ctx, size_t n, size_t q, const uint8_t* d_sigma1,
                                       const uint8_t* d_sigma2, const uint8_t* d_msgs, const uint8_t* d_vk_X,
                                       const uint8_t* d_vk_Y, uint8_t* d_verdicts, uint8_t* d_gt_or_null,
                                       void* stream);

/* Concurrent verify batches on one context: with `slots` = K > 1, cc_verify_batch_device,
 * cc_verify_batch_pervk_device, cc_pok_verify_batch_device, cc_pok_verify_batch_pervk_device,
 * cc_rlc_partial_device and cc_pok_rlc_partial_device calls take K
 * workspace slots round-robin (each slot its own prep SoA, flags, Miller values, PoK d J tables and RLC
 * delta/fold buffers; the verkey tables are shared)
 * and are ordered only after the context's earlier work (tables, params) and the same slot's previous
 * batch — so K batches issued on K caller streams overlap on the device (one batch's kernel tails with
 * the next batch's kernels).  Every other
 * entry point, and cc_set_params / cc_set_verkey, first waits for the slots' batches.  The per-phase
 * timing (cc_last_timing) is meaningful with one slot only.  slots: 1 (default, every call ordered
 * against every other) .. 8.  cc_concurrency reports the current value. */
cc_status cc_set_concurrency(cc_ctx* ctx, int slots);
cc_status cc_concurrency(const cc_ctx* ctx, int* slots);

/* RLC batch mode, multi-GPU form.  Each GPU reduces its shard to one partial of
 * CC_RLC_PARTIAL_WORDS u32 (= cc_rlc_partial_words(): the Fp12 Miller product in the library's
 * Montgomery words, a fall-back flag, and the shard's 16 fold window sums, affine with identity
 * flags); the caller gathers the partials of all GPUs (RCCL all-gather over xGMI, or any transport)
 * and every GPU finishes with 16 window pairs per partial and ONE final exponentiation:
 *   cc_rlc_partial_device: deltas = ChaCha20(seed32, base_index + i), i < n (shared verkey only);
 *                          d_partial: CC_RLC_PARTIAL_WORDS x u32 device buffer; n = 0 (an empty
 *                          shard) writes the neutral partial (Fp12 one, flag clear, identity window
 *                          sums) so the rank still joins the gather.
 *   cc_rlc_finish_device : nparts partials (nparts x CC_RLC_PARTIAL_WORDS u32, device): their window
 *                          pairs, the product, the final exponentiation; *d_accept = 1 iff the whole
 *                          batch verifies (then every per-credential verdict is 1); 0 means "fall back
 *                          to per-credential verification" (a bad or identity credential somewhere).
 *                          d_gt optional (576 B, GT of the combined product).  Needs the verkey of the
 *                          partials (its g~ multiples); a cc_set_verkey waits for running finishes.
 * Both are asynchronous on `stream` (NULL: the context stream).  The partial is ordered against the
 * context's other work; the finish owns its buffers and is NOT, so on a second stream it may overlap
 * the next batch's partial (the caller orders d_partials before it, and two finishes of one context
 * one after the other); with cc_set_concurrency(K) successive partials take K slots and overlap too.  cc_verify_batch(..., rlc = 1) runs the single-GPU form with a fresh seed
 * from /dev/urandom and falls back by itself. */
#define CC_RLC_PARTIAL_WORDS 929
int cc_rlc_partial_words(void);
cc_status cc_rlc_partial_device(cc_ctx* ctx, size_t n, size_t q, uint64_t base_index, const uint8_t* seed32,
                                const uint8_t* d_sigma1, const uint8_t* d_sigma2, const uint8_t* d_msgs,
                                uint32_t* d_partial, void* stream);
cc_status cc_rlc_finish_device(cc_ctx* ctx, size_t nparts, const uint32_t* d_partials, uint8_t* d_accept,
                               uint8_t* d_gt_or_null, void* stream);

/* RLC locate: the batch is checked in segments, and only the segments whose own RLC check fails are
 * verified per credential, so a bad credential costs its segment's re-verification, not the batch's
 * (rlc = 1 above falls back over the WHOLE batch).  Every segment is an RLC check of its own with
 * independent deltas, so the 2^-127 bound holds per segment; verdicts always equal rlc = 0's.  Shared
 * verkey only; no GT output; these calls take no concurrency slot (cc_set_concurrency): like every
 * other entry point they wait for the slots' batches and are ordered on the context's stream.
 *   cc_rlc_partial_seg_device : cc_rlc_partial_device in one pass for every segment of `seg`
 *                               credentials: S = ceil(n / seg) partials (S x CC_RLC_PARTIAL_WORDS u32),
 *                               partial s covering credentials [s seg, min(n, (s + 1) seg)) and equal to
 *                               what cc_rlc_partial_device(hi - lo, base_index + s seg, seed32, slice)
 *                               writes.  seg: a power of two, 4 <= seg <= CC_MAX_BATCH, and S <=
 *                               CC_MAX_PARTS, else CC_ERR_DECODE; n = 0: CC_OK, nothing written; the other
 *                               errors as cc_rlc_partial_device.
 *   cc_rlc_finish_each_device : cc_rlc_finish_device(1, partial s) for every one of nparts partials in
 *                               one launch sequence: d_accept nparts bytes, d_gt_or_null nparts x 576 B.
 *                               Takes any partials of the layout (segment, shard or neutral ones); its
 *                               buffers and ordering are cc_rlc_finish_device's (finishes of either kind
 *                               run in call order; a cc_set_verkey waits for them).
 *   cc_verify_batch_locate_device : the segmented partial, the per-partial finish, then ONE per-credential
 *                               launch sequence over the rejected segments only (their rows compacted;
 *                               every segment rejected: the batch verified in place); d_verdicts n bytes.
 *                               seg = 0: the library's default for the context's group mode
 *                               (CC_LOCATE_SEG_DEFAULT_G2 / _G1).  The call downloads the S accept bytes
 *                               to decide what to launch, so it SYNCHRONISES `stream` ONCE; the recheck is
 *                               left queued (synchronise before reading verdicts).  stats3_or_null: three
 *                               HOST words written before the call returns: segments, rejected segments,
 *                               credentials rechecked.
 *   cc_verify_batch_locate    : the host form (host arrays, a fresh seed as rlc = 1 draws it); on a device
 *                               set every device locates inside its own shard and there is no collective.
 * The defaults come from tools/bench_rlc_locate.py on config 3's per-GPU shape (131,072 credentials, q =
 * 16, one MI355X): per mode the segment length with the best one-bad-credential rate among those whose
 * all-valid rate stays within twice the run's spread of cc_rlc_partial_device + cc_rlc_finish_device's
 * (SigG2 4,096: 0.6 % below; SigG1 1,024: 3.0 % below).  DESIGN.md "RLC locate" has the table. */
#define CC_LOCATE_SEG_DEFAULT_G2 4096
#define CC_LOCATE_SEG_DEFAULT_G1 1024
cc_status cc_rlc_partial_seg_device(cc_ctx* ctx, size_t n, size_t q, size_t seg, uint64_t base_index,
                                    const uint8_t* seed32, const uint8_t* d_sigma1, const uint8_t* d_sigma2,
                                    const uint8_t* d_msgs, uint32_t* d_partials, void* stream);
cc_status cc_rlc_finish_each_device(cc_ctx* ctx, size_t nparts, const uint32_t* d_partials, uint8_t* d_accept,
                                    uint8_t* d_gt_or_null, void* stream);
cc_status cc_verify_batch_locate_device(cc_ctx* ctx, size_t n, size_t q, size_t seg, const uint8_t* seed32,
                                        const uint8_t* d_sigma1, const uint8_t* d_sigma2, const uint8_t* d_msgs,
                                        uint8_t* d_verdicts, uint32_t* stats3_or_null, void* stream);
cc_status cc_verify_batch_locate(cc_ctx* ctx, size_t n, size_t q, size_t seg, const uint8_t* sigma1,
                                 const uint8_t* sigma2, const uint8_t* msgs, uint8_t* verdicts,
                                 uint32_t* stats3_or_null);

/* Batch Signature::aggregate: n independent aggregations of `len` (id, Signature) entries each;
 * only the first t entries are used, sigma_1 comes from entry 0, Lagrange over the de-duplicated
 * id set (signature.rs:448-470).  ids: n x len; sigma1/sigma2: n x len encodings;
 * out_sigma1/out_sigma2: n encodings. */
cc_status cc_signature_aggregate_batch(cc_ctx* ctx, size_t n, size_t len, size_t t, const uint64_t* ids,
                                       const uint8_t* sigma1, const uint8_t* sigma2, uint8_t* out_sigma1,
                                       uint8_t* out_sigma2);

/* Batch Verkey::aggregate (signature.rs:483-526): X: n x len, Y: n x len x q; outX: n; outY: n x q. */
cc_status cc_verkey_aggregate_batch(cc_ctx* ctx, size_t n, size_t len, size_t t, size_t q, const uint64_t* ids,
                                    const uint8_t* X, const uint8_t* Y, uint8_t* outX, uint8_t* outY);

/* Device-buffer form of cc_signature_aggregate_batch (inputs resident in HBM; the timed path of
 * BASELINE config 4).  Asynchronous on `stream` (NULL: the context stream). */
cc_status cc_signature_aggregate_batch_device(cc_ctx* ctx, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                              const uint8_t* d_sigma1, const uint8_t* d_sigma2,
                                              uint8_t* d_out_sigma1, uint8_t* d_out_sigma2, void* stream);

/* Issuer table for Verkey::aggregate at scale (BASELINE config 4: t = 67 of n = 100 issuers).  The
 * n_issuers verkeys (X: n_issuers x OtherGroup, Y: n_issuers x q x OtherGroup) and their signer ids
 * (unique) are decoded once and given fixed-base window tables in HBM (one-time cost; the widest
 * window in {16, 13, 12, 10, 8} whose tables fit 16 GiB and half the free HBM — 13-bit, 11 GB, for
 * 100 issuers x 7 G1 keys — or the width forced by cc_set_table_bits); a batch then passes only id
 * lists.  A failed call leaves no issuer table (CC_ERR_STATE afterwards).
 * cc_verkey_aggregate_ids(_device) computes, per credential, exactly
 * Verkey::aggregate(t, [(id_k, &issuer[id_k])]) (signature.rs:483-526): first t entries, Lagrange
 * over the de-duplicated id set.  ids: n x len.  An id without an issuer verkey (the reference would
 * index a missing key): the host form returns CC_ERR_DECODE before launching; the device form writes
 * the identity encoding for the affected outputs and raises the context's device error word
 * (CC_DEVERR_UNKNOWN_ID), which cc_device_error reads. */
cc_status cc_set_issuers(cc_ctx* ctx, size_t n_issuers, size_t q, const uint64_t* ids, const uint8_t* X,
                         const uint8_t* Y);
cc_status cc_verkey_aggregate_ids(cc_ctx* ctx, size_t n, size_t len, size_t t, const uint64_t* ids, uint8_t* outX,
                                  uint8_t* outY);
cc_status cc_verkey_aggregate_ids_device(cc_ctx* ctx, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                         uint8_t* d_outX, uint8_t* d_outY, void* stream);

/* Both aggregations of the same credentials, as a verifier holding per-credential shares does them:
 * Signature::aggregate(t, [(id_k, sig_k)]) (signature.rs:448-470) and Verkey::aggregate(t, [(id_k,
 * issuer[id_k])]) (signature.rs:483-526) over ONE id list per credential, so the Lagrange coefficients
 * (signature.rs:454-463 = 496-509) are computed once.  Outputs and errors as the two calls above
 * (device error word as cc_verkey_aggregate_ids_device).  Asynchronous on `stream`. */
cc_status cc_aggregate_credential_batch_device(cc_ctx* ctx, size_t n, size_t len, size_t t, const uint64_t* d_ids,
                                               const uint8_t* d_sigma1, const uint8_t* d_sigma2,
                                               uint8_t* d_out_sigma1, uint8_t* d_out_sigma2, uint8_t* d_outX,
                                               uint8_t* d_outY, void* stream);

/* Argument errors that only the device can see (ids checked inside a kernel of a *_device call):
 * synchronises `stream` (NULL: the context stream), returns the OR of the CC_DEVERR_* bits raised since
 * the last read in *out, and clears them. */
#define CC_DEVERR_UNKNOWN_ID 1u
cc_status cc_device_error(cc_ctx* ctx, void* stream, uint32_t* out);

/* Batch PoKOfSignatureProof::verify against the shared verkey and params.
 *   sigma1, sigma2  : n x SignatureGroup (sigma'_1, sigma'_2)
 *   J, T            : n x OtherGroup (J and the Schnorr commitment)
 *   responses       : n x (q - r + 1) x 48 B, order [g~, Y~_i for hidden i ascending]
 *   chal            : n x 48 B
 *   revealed_idx    : r indices (shared by the batch, ascending, < q)
 *   revealed_msgs   : n x r x 48 B
 * CC_ERR_BASES_EXPS if nresp != q - r + 1 (ps_sig returns UnequalNoOfBasesExponents). */
cc_status cc_pok_verify_batch(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* sigma1,
                              const uint8_t* sigma2, const uint8_t* J, const uint8_t* T, const uint8_t* responses,
                              const uint8_t* chal, const uint64_t* revealed_idx, const uint8_t* revealed_msgs,
                              uint8_t* verdicts, uint8_t* gt_or_null);

/* Same, with the per-proof buffers already in device memory (the timed bench path, config 5);
 * revealed_idx stays a host array of r indices.  Asynchronous on `stream` (NULL: context stream). */
cc_status cc_pok_verify_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* d_sigma1,
                                     const uint8_t* d_sigma2, const uint8_t* d_J, const uint8_t* d_T,
                                     const uint8_t* d_responses, const uint8_t* d_chal, const uint64_t* revealed_idx,
                                     const uint8_t* d_revealed_msgs, uint8_t* d_verdicts, uint8_t* d_gt_or_null,
                                     void* stream);

/* PoKOfSignatureProof::verify(&vk_i, &params, revealed_msgs, &chal) for each proof i with ITS OWN verkey
 * (src/pok_sig.rs:103-105 takes the verkey per call): a verifier whose credentials come from different
 * authority subsets holds one aggregated verkey per credential (what cc_verkey_aggregate_ids_device and
 * cc_aggregate_credential_batch_device write).
 *   d_vk_X : n x OtherGroup        d_vk_Y : n x q x OtherGroup   (cc_verify_batch_pervk_device's layout)
 * Every other argument has the meaning, order and encoding it has in cc_pok_verify_batch_device:
 * revealed_idx is a host array shared by the batch (any order, unique, < q), responses are ordered
 * [g~, Y~_i for hidden i ascending], revealed messages are in revealed_idx order.  Per proof:
 *   resp_0 g~ + sum_hidden resp_j Y~_i,j + chal J - T == O   and   e(sigma'_1, X~_i + J +
 *   sum_revealed m_z Y~_i,idx[z]) e(-sigma'_2, g~) == 1,
 * with the reference's handling of every input: a point that does not decode is the identity, scalars
 * are reduced mod r, bases and J need not lie in the order-r subgroup.
 * Needs cc_set_params only: no cc_set_verkey, and q is not compared with a loaded verkey.
 * Checks, in order and before the n = 0 shortcut: NULL context, or a NULL buffer with n > 0 (d_vk_X, and
 * d_vk_Y when q > 0, among them) -> CC_ERR_DECODE; no params -> CC_ERR_STATE; q > 4096 -> CC_ERR_DECODE;
 * a revealed index >= q -> CC_ERR_LEN, a repeated one -> CC_ERR_DECODE; nresp != q - r + 1 ->
 * CC_ERR_BASES_EXPS; n > CC_MAX_BATCH -> CC_ERR_DECODE.  n = 0 is then a no-op (buffers may be NULL).
 * Asynchronous on `stream` (NULL: the context stream); takes a concurrency slot (cc_set_concurrency)
 * as the two calls it combines do.  Device memory: the prep's per-proof window tables, 8 (q + 2) points
 * a proof — at q = 32, 67,584 B a proof in CC_SIG_G2 and 132,864 B in CC_SIG_G1 (4.43 GB and 8.71 GB at
 * 65,536 proofs), held by the context (per slot) until it is destroyed.
 * cc_pok_verify_batch_pervk: the same with host pointers: one upload, the device form, one download. */
cc_status cc_pok_verify_batch_pervk_device(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp,
                                           const uint8_t* d_sigma1, const uint8_t* d_sigma2, const uint8_t* d_J,
                                           const uint8_t* d_T, const uint8_t* d_responses, const uint8_t* d_chal,
                                           const uint64_t* revealed_idx, const uint8_t* d_revealed_msgs,
                                           const uint8_t* d_vk_X, const uint8_t* d_vk_Y, uint8_t* d_verdicts,
                                           uint8_t* d_gt_or_null, void* stream);
cc_status cc_pok_verify_batch_pervk(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* sigma1,
                                    const uint8_t* sigma2, const uint8_t* J, const uint8_t* T,
                                    const uint8_t* responses, const uint8_t* chal, const uint64_t* revealed_idx,
                                    const uint8_t* revealed_msgs, const uint8_t* vk_X, const uint8_t* vk_Y,
                                    uint8_t* verdicts, uint8_t* gt_or_null);

/* Holder side: ps_sig PoKOfSignature::init / gen_proof [EXT] (reference src/pok_sig.rs:80-100) and
 * BlindSignature::unblind (src/signature.rs:436-443), what cc_pok_verify_batch consumes.
 *
 * PoKOfSignature::init for n credentials under the shared verkey and params.
 *   sigma1, sigma2 : n x SignatureGroup      msgs : n x q x 48
 *   revealed_idx   : r indices (host array, rules of cc_pok_verify_batch)
 *   rand           : n x (nresp + 2) x 48 = r1 | r2 | b_0 .. b_{nresp-1}   (caller's randomness)
 *   out: sigma'_1 = r1 s1, sigma'_2 = r1 (s2 + r2 s1)      (n x SignatureGroup each)
 *        J = r2 g~ + sum_hidden m_i Y~_i,  T = b_0 g~ + sum_hidden b_j Y~_i   (n x OtherGroup each)
 *   bases and responses ordered [g~, Y~_i for hidden i ascending], as cc_pok_verify_batch reads them
 * Checks, in cc_pok_verify_batch_device's order and before the n = 0 shortcut: NULL context, or a NULL
 * buffer with n > 0, or NULL revealed_idx with r > 0: CC_ERR_DECODE; no params / verkey: CC_ERR_STATE
 * (init only; gen_proof and unblind need neither); q != the verkey's q: CC_ERR_LEN (gen_proof: q >
 * CC_MAX_Q is CC_ERR_DECODE); an index >= q: CC_ERR_LEN, a repeated index: CC_ERR_DECODE; nresp !=
 * q - r + 1: CC_ERR_BASES_EXPS; n > CC_MAX_BATCH: CC_ERR_DECODE.
 * Scalars are reduced mod r, a bad prefix or an off-curve point decodes to the identity, an identity
 * result (r1 = 0, sigma_2 = -r2 sigma_1, all blindings 0) is written as the identity encoding; nothing
 * is rejected that ps_sig would not reject.
 * The *_device forms take device pointers (revealed_idx stays a host array), are asynchronous on
 * `stream` (NULL: the context stream) and take no concurrency slot: they first wait for the slots'
 * batches.  A device set forwards to its first device.
 * Secrets: the host forms copy rand (r1, r2, the blindings) and sk to the device and build the digits of
 * r1, r1 r2 and -sk in device scratch; they overwrite those device copies with zeros before
 * returning.  The *_device forms read the caller's buffers in place; their scratch (the digits of r1
 * and r1 r2) stays until the next call overwrites it or the context is destroyed. */
cc_status cc_pok_init_batch(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* sigma1,
                            const uint8_t* sigma2, const uint8_t* msgs, const uint64_t* revealed_idx,
                            const uint8_t* rand, uint8_t* out_sigma1, uint8_t* out_sigma2, uint8_t* out_J,
                            uint8_t* out_T);
cc_status cc_pok_init_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* d_sigma1,
                                   const uint8_t* d_sigma2, const uint8_t* d_msgs, const uint64_t* revealed_idx,
                                   const uint8_t* d_rand, uint8_t* d_out_sigma1, uint8_t* d_out_sigma2,
                                   uint8_t* d_out_J, uint8_t* d_out_T, void* stream);

/* gen_proof: responses[0] = b_0 - chal r2, responses[1 + j] = b_{1+j} - chal m_hidden_j  (mod r);
 * msgs, rand as cc_pok_init_batch, chal n x 48, out_responses n x nresp x 48. */
cc_status cc_pok_gen_proof_batch(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* msgs,
                                 const uint64_t* revealed_idx, const uint8_t* rand, const uint8_t* chal,
                                 uint8_t* out_responses);
cc_status cc_pok_gen_proof_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp,
                                        const uint8_t* d_msgs, const uint64_t* revealed_idx, const uint8_t* d_rand,
                                        const uint8_t* d_chal, uint8_t* d_out_responses, void* stream);

/* BlindSignature::unblind: sigma_2 = c2 - sk c1, one ElGamal key per row (c1, c2: n x SignatureGroup,
 * sk: n x 48); sigma_1 is the blind signature's h.  An identity c1 or sk = 0 gives c2 back. */
cc_status cc_unblind_batch(cc_ctx* ctx, size_t n, const uint8_t* c1, const uint8_t* c2, const uint8_t* sk,
                           uint8_t* out_sigma2);

/* RLC batch mode for PoKOfSignatureProof::verify (shared verkey).  The proof's pairing equation
 * e(sigma'_1, J') * e(-sigma'_2, g~) == 1, J' = X~ + J + sum_revealed m_i Y~_i, has the shape of
 * Signature::verify's, so a batch is checked as one delta-weighted pairing product, with the
 * deltas, the partial format and the finish of the RLC block above; the Schnorr relation costs no
 * pairing and is checked per proof, exactly.  Contract: a batch is accepted only if every proof's
 * Schnorr relation holds exactly and the delta-weighted pairing product is one; a forged batch passes
 * with probability <= 2^-127.  A sigma' that is the identity or outside the subgroup, a J outside the
 * subgroup, a failed Schnorr relation or a verkey / g~ outside the subgroup raise the partial's
 * fall-back flag: the finish then rejects and the caller verifies per proof, so verdicts never change.
 *   cc_pok_rlc_partial_device: arguments and errors of cc_pok_verify_batch_device, deltas =
 *                              ChaCha20(seed32, base_index + i); d_partial: CC_RLC_PARTIAL_WORDS x u32
 *                              device buffer, finished by cc_rlc_finish_device, alone or with the partials
 *                              of the other shards of the same PoK batch; n = 0 writes the neutral
 *                              partial.  Asynchronous on `stream` (NULL: the context stream); takes a
 *                              concurrency slot as cc_rlc_partial_device does (cc_set_concurrency).
 *   cc_pok_verify_batch_rlc  : cc_pok_verify_batch without the GT output: one upload, partial + finish
 *                              with a fresh seed from /dev/urandom; all-ones verdicts on accept, else
 *                              the per-proof path on the buffers already on the device.  Verdicts always
 *                              equal cc_pok_verify_batch's. */
cc_status cc_pok_rlc_partial_device(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, uint64_t base_index,
                                    const uint8_t* seed32, const uint8_t* d_sigma1, const uint8_t* d_sigma2,
                                    const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_responses,
                                    const uint8_t* d_chal, const uint64_t* revealed_idx,
                                    const uint8_t* d_revealed_msgs, uint32_t* d_partial, void* stream);
cc_status cc_pok_verify_batch_rlc(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, const uint8_t* sigma1,
                                  const uint8_t* sigma2, const uint8_t* J, const uint8_t* T, const uint8_t* responses,
                                  const uint8_t* chal, const uint64_t* revealed_idx, const uint8_t* revealed_msgs,
                                  uint8_t* verdicts);

/* PoK RLC locate: the locate mode above for PoKOfSignatureProof::verify.  The batch is checked in segments
 * of `seg` proofs, each an RLC check of its own (independent deltas: a forged segment passes with
 * probability <= 2^-127 per segment, and every proof's Schnorr relation is still checked exactly), and only
 * the segments whose check fails are verified per proof; verdicts always equal cc_pok_verify_batch's.  What
 * raises segment s's fall-back flag, and nothing outside it: a proof of the segment whose sigma'_1 or
 * sigma'_2 is the identity or outside the subgroup (SigG2's sigma'_1 test comes from the Miller loop's own T:
 * two proofs a loop, four past the two-proof limit, and a loop never straddles two segments), whose Schnorr
 * relation fails, or whose J lies outside the subgroup.  A verkey component or g~ outside the subgroup flags
 * EVERY segment (the batch is then verified in place).  A proof that fails only the pairing equation raises
 * no flag: its segment's product is not one.  Shared verkey only; no GT output; these calls take no
 * concurrency slot (cc_set_concurrency): they wait for the slots' batches and are ordered on the context's
 * stream, as the signature locate calls are.
 *   cc_pok_rlc_partial_seg_device : cc_pok_rlc_partial_device in one pass for every segment: S = ceil(n / seg)
 *                               partials (S x CC_RLC_PARTIAL_WORDS u32, finished by cc_rlc_finish_each_device),
 *                               partial s covering proofs [s seg, min(n, (s + 1) seg)) and equal to what
 *                               cc_pok_rlc_partial_device(hi - lo, base_index + s seg, seed32, slice) writes
 *                               (word for word while both take the same Miller loop: up to 65,536 proofs on
 *                               an MI355X; beyond, the same decisions).  Errors: those of
 *                               cc_pok_rlc_partial_device in its order, then seg: a power of two, 4 <= seg <=
 *                               CC_MAX_BATCH, and S <= CC_MAX_PARTS, else CC_ERR_DECODE.  n = 0: CC_OK, nothing
 *                               written.
 *   cc_pok_verify_batch_locate_device : the segmented partial, the per-partial finish, then ONE
 *                               cc_pok_verify_batch_device launch sequence over the rejected segments only
 *                               (all seven per-proof arrays compacted device-to-device, a run of adjacent
 *                               rejected segments at a time; every segment rejected: the batch verified in
 *                               place); d_verdicts n bytes.  seg = 0: the library's default for the context's
 *                               group mode (CC_POK_LOCATE_SEG_DEFAULT_G2 / _G1).  SYNCHRONISES `stream` ONCE
 *                               (the download of the S accept bytes); the recheck is left queued.
 *                               stats3_or_null: as cc_verify_batch_locate_device (segments, rejected segments,
 *                               proofs rechecked; HOST words).
 *   cc_pok_verify_batch_locate : the host form: one upload, a fresh seed from /dev/urandom, the device form,
 *                               one download.  A device set forwards to its first device, as every PoK host
 *                               form does.
 * The defaults come from tools/bench_pok_locate.py on config 5's shape (65,536 proofs, q = 32, 8 revealed,
 * one MI355X) by the rule of CC_LOCATE_SEG_DEFAULT_*: per mode the segment length with the best
 * one-bad-proof rate among those whose all-valid rate stays within twice the run's spread of
 * cc_pok_rlc_partial_device + cc_rlc_finish_device's (SigG2 1,024: 2.0 % below; SigG1 1,024: 1.0 % below).
 * There one bad proof costs 1.72x less time than the RLC pass plus the per-proof pass in both modes, but the
 * per-proof path alone is still faster on such a batch (locate reaches 0.92 of its rate in SigG2, 0.85 in
 * SigG1).  DESIGN.md "PoK RLC locate" has the table. */
#define CC_POK_LOCATE_SEG_DEFAULT_G2 1024
#define CC_POK_LOCATE_SEG_DEFAULT_G1 1024
cc_status cc_pok_rlc_partial_seg_device(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, size_t seg,
                                        uint64_t base_index, const uint8_t* seed32, const uint8_t* d_sigma1,
                                        const uint8_t* d_sigma2, const uint8_t* d_J, const uint8_t* d_T,
                                        const uint8_t* d_responses, const uint8_t* d_chal,
                                        const uint64_t* revealed_idx, const uint8_t* d_revealed_msgs,
                                        uint32_t* d_partials, void* stream);
cc_status cc_pok_verify_batch_locate_device(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, size_t seg,
                                            const uint8_t* seed32, const uint8_t* d_sigma1, const uint8_t* d_sigma2,
                                            const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_responses,
                                            const uint8_t* d_chal, const uint64_t* revealed_idx,
                                            const uint8_t* d_revealed_msgs, uint8_t* d_verdicts,
                                            uint32_t* stats3_or_null, void* stream);
cc_status cc_pok_verify_batch_locate(cc_ctx* ctx, size_t n, size_t q, size_t r, size_t nresp, size_t seg,
                                     const uint8_t* sigma1, const uint8_t* sigma2, const uint8_t* J, const uint8_t* T,
                                     const uint8_t* responses, const uint8_t* chal, const uint64_t* revealed_idx,
                                     const uint8_t* revealed_msgs, uint8_t* verdicts, uint32_t* stats3_or_null);

/* Codec check: decode n encodings of `group` (1 = G1 97 B, 2 = G2 192 B) and
 * report per point 0 = identity (AMCL maps a bad prefix / off-curve point to infinity), 1 = on the
 * curve but outside the order-r subgroup, 2 = in G1 / G2.  The reference never tests membership on
 * verify, so cc_verify_batch keeps its semantics; the RLC batch mode uses the same tests internally
 * (a sigma or verkey point outside the subgroup makes the batch fall back to per-credential).
 * Tests: G1 phi(P) == -[x^2] P, G2 psi(Q) == [x] Q (eprint 2021/1130, 2022/352). */
cc_status cc_subgroup_check(cc_ctx* ctx, int group, size_t n, const uint8_t* points, uint8_t* status);

/* Batched amcl_wrapper `from_msg_hash`: n messages, message i =
 * data[offsets[i] .. offsets[i+1]) (offsets: n + 1 entries, offsets[0] = 0), each hashed with
 * SHAKE256 to 48 bytes and mapped to `group` (1 = G1, 2 = G2) by AMCL's try-and-increment `mapit`
 * with cofactor clearing; out: n encodings.  Params::new (signature.rs:22-32) hashes label || " : g",
 * " : g_tilde", " : y" || i; SignatureRequest::compute_h (signature.rs:197-206) hashes
 * commitment.to_bytes() || m_i.to_bytes().  Parity unpinned (AMCL restated, see oracle/).
 * cc_hash_msg: the 48-byte SHAKE256 digests alone (amcl_wrapper hash_msg). */
cc_status cc_hash_to_curve(cc_ctx* ctx, int group, size_t n, const uint8_t* data, const uint64_t* offsets,
                           uint8_t* out);
cc_status cc_hash_msg(cc_ctx* ctx, size_t n, const uint8_t* data, const uint64_t* offsets, uint8_t* out48);

/* Issuer-side batch, n signature requests with k hidden of q messages,
 * SignatureGroup encodings:
 *   cc_blind_sign_batch  : BlindSignature::new (signature.rs:382-433) under one issuer key
 *       commitment n x SG | known n x (q-k) x 48 | ciphertexts n x k x (c1, c2) | x 48 | y q x 48
 *       -> out_h (= compute_h), out_c1, out_c2 (n x SG each)
 *   cc_sigreq_verify_batch : SignatureRequestProof::verify (signature.rs:324-377), verdicts n bytes;
 *       g and h[0..k) are the Params' SignatureGroup generators; elgamal_pk n x SG; chal n x 48;
 *       proofs n x cc_sigreq_proof_bytes(ctx, k) bytes, per request:
 *         T_sk | r_sk | T_comm | r_comm[k+1] | k x (T_1 | r_1 | T_2 | r_2a | r_2b)
 *       (T = Schnorr commitment encodings, r = 48-byte responses).
 * CC_ERR_LEN if k > q (the reference's assert_eq!). */
cc_status cc_blind_sign_batch(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* commitment,
                              const uint8_t* known, const uint8_t* ciphertexts, const uint8_t* x, const uint8_t* y,
                              uint8_t* out_h, uint8_t* out_c1, uint8_t* out_c2);
size_t cc_sigreq_proof_bytes(const cc_ctx* ctx, size_t k);
cc_status cc_sigreq_verify_batch(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* g, const uint8_t* h,
                                 const uint8_t* commitment, const uint8_t* known, const uint8_t* ciphertexts,
                                 const uint8_t* elgamal_pk, const uint8_t* proofs, const uint8_t* chal,
                                 uint8_t* verdicts);

/* Holder side of issuance: SignatureRequest::new ("PrepareBlindSign", signature.rs:124-192) and
 * SignatureRequestPoK::init / gen_proof (216-320), what cc_sigreq_verify_batch and cc_blind_sign_batch
 * consume.  SG = a SignatureGroup encoding, pb = cc_sigreq_proof_bytes(ctx, k).
 *
 * cc_set_request_params binds Params.g (one SG) and Params.h (q x SG) and builds SignatureGroup
 * fixed-base window tables for [h_0 .. h_{q-1}, g] (g is table base q).  table_bits in 8..16 forces the
 * window width (a width that does not fit the free HBM: CC_ERR_HIP); 0 takes the widest of {16, 13, 12,
 * 10, 8} whose tables fit min(4 GiB, half the free HBM), 8 bits if the allocation fails.  The tables are
 * the context's own: the verkey and issuer tables and cc_set_table_bits are untouched.  An identity or
 * undecodable base is skipped in every sum.  NULL ctx, g or h, q = 0, q > CC_MAX_Q or table_bits outside
 * {0, 8..16}: CC_ERR_DECODE.  A failed call leaves the context without request params.
 *
 * cc_sigreq_new_batch, n requests with k hidden of q messages:
 *   msgs n x q x 48 | elgamal_pk n x SG | rand n x (k + 1) x 48 = r | k_0 .. k_{k-1}  (the order of the
 *   reference's returned randomness)
 *   -> commitment = sum_{i<k} m_i h_i + r g,  h = compute_h(commitment, m_k .. m_{q-1}) (also for k = 0),
 *      ciphertexts n x k x (c1_i = k_i g, c2_i = k_i pk + m_i h)
 * cc_sigreq_pok_init_batch, h = out_h of new:
 *   blind n x (3k + 2) x 48 = b_sk | hb_0 .. hb_{k-1} | b_r | k x (b1_i | b2_i)
 *   -> the T fields of the proof record (layout at cc_sigreq_verify_batch): T_sk = b_sk g,
 *      T_comm = sum hb_i h_i + b_r g, T_1i = b1_i g, T_2i = b2_i pk + hb_i h; the response fields zeroed.
 * cc_sigreq_pok_gen_proof_batch writes only the response fields, each b - chal * secret mod r:
 *   r_sk = b_sk - c sk, r_comm[i] = hb_i - c m_i, r_comm[k] = b_r - c r, r_1 = b1_i - c k_i,
 *   r_2a = b2_i - c k_i, r_2b = hb_i - c m_i  (elgamal_sk, chal: n x 48).  After it `proofs` is what
 *   cc_sigreq_verify_batch accepts.
 * Checks, in this order and before the n = 0 shortcut: NULL context: CC_ERR_DECODE; a NULL buffer the
 * call would read or write with n > 0 (with k = 0 elgamal_pk, h and the ciphertexts may be NULL):
 * CC_ERR_DECODE; no request params: CC_ERR_STATE (new, init); q != the request params' q: CC_ERR_LEN
 * (gen_proof needs no params: q > CC_MAX_Q is CC_ERR_DECODE); k > q: CC_ERR_LEN; n > CC_MAX_BATCH:
 * CC_ERR_DECODE.
 * Scalars are reduced mod r, a bad prefix or an off-curve elgamal_pk or h decodes to the identity, an
 * identity result (k_i = 0, all blindings 0) is written as the identity encoding; nothing is rejected
 * that the reference would not reject.
 * The *_device forms take device pointers, are asynchronous on `stream` (NULL: the context stream) and
 * take no concurrency slot: they first wait for the slots' batches.  A device set forwards to its first
 * device.  (The 2^-4096 event of compute_h's try-and-increment giving up is CC_ERR_DECODE from the host
 * form of new; the device form does not report it.)
 * Secrets: the host forms copy msgs, rand, blind and elgamal_sk to the device and build the digits of
 * k_i, m_i, b2_i and hb_i in device scratch; they overwrite those device copies with zeros before
 * returning.  The *_device forms read the caller's buffers in place; their scratch (those digits) stays
 * until the next call overwrites it or the context is destroyed. */
cc_status cc_set_request_params(cc_ctx* ctx, size_t q, const uint8_t* g, const uint8_t* h, int table_bits);
cc_status cc_sigreq_new_batch(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* msgs,
                              const uint8_t* elgamal_pk, const uint8_t* rand, uint8_t* out_commitment,
                              uint8_t* out_h, uint8_t* out_ciphertexts);
cc_status cc_sigreq_new_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* d_msgs,
                                     const uint8_t* d_elgamal_pk, const uint8_t* d_rand, uint8_t* d_out_commitment,
                                     uint8_t* d_out_h, uint8_t* d_out_ciphertexts, void* stream);
cc_status cc_sigreq_pok_init_batch(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* h,
                                   const uint8_t* elgamal_pk, const uint8_t* blind, uint8_t* out_proofs);
cc_status cc_sigreq_pok_init_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* d_h,
                                          const uint8_t* d_elgamal_pk, const uint8_t* d_blind, uint8_t* d_out_proofs,
                                          void* stream);
cc_status cc_sigreq_pok_gen_proof_batch(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* msgs,
                                        const uint8_t* rand, const uint8_t* blind, const uint8_t* elgamal_sk,
                                        const uint8_t* chal, uint8_t* proofs);
cc_status cc_sigreq_pok_gen_proof_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* d_msgs,
                                               const uint8_t* d_rand, const uint8_t* d_blind,
                                               const uint8_t* d_elgamal_sk, const uint8_t* d_chal, uint8_t* d_proofs,
                                               void* stream);

/* Issuer side of issuance with every input in HBM: the device forms of cc_sigreq_verify_batch and
 * cc_blind_sign_batch (buffer layouts and the proof record as there), asynchronous on `stream` (NULL: the
 * context stream), no host round trip.  They take no concurrency slot: they first wait for the slots'
 * batches.  A device set forwards to its first device.
 *
 * cc_sigreq_verify_batch_device reads g and h_0 .. h_{k-1} from the context's request params
 * (cc_set_request_params) and gives, per request, exactly the verdict of cc_sigreq_verify_batch called
 * with those: the fixed-base terms r g, sum r_i h_i come from the request params' window tables with no
 * doubling, the variable-base terms (c pk, c commitment, c c1_i, r_2a pk + r_2b h + c c2_i) from one
 * per-request table of signed 4-bit windows (no endomorphism: a key or ciphertext outside the subgroup
 * gives its integer multiple).  With d_out_h set it also writes h = compute_h(commitment, known) of every
 * request, accepted or not: the bytes cc_blind_sign_batch returns in out_h.
 *
 * cc_blind_sign_batch_device gives the bytes of cc_blind_sign_batch.  With d_h set it takes h from there
 * (what the verify wrote) instead of hashing again, and d_commitment may then be NULL; with d_h NULL it
 * computes h from d_commitment and d_known.  Either way h is written to d_out_h (d_out_h == d_h is
 * allowed).  It needs neither request params nor a verkey, only the context: compute_h is a hash, and the
 * two sums run over each request's own ciphertexts.  x (48 B) and y (q x 48 B) are HOST arrays, one issuer
 * key for the batch; the call copies them before it returns and queues, behind its work, the zeroing of
 * its device copies of x, y, the tasks' scalars and their digits.
 *
 * Checks, in this order and before the n = 0 shortcut: NULL context (sign: NULL x, or NULL y with q > 0):
 * CC_ERR_DECODE; a NULL buffer the call would read or write with n > 0 (k = 0: the ciphertexts may be
 * NULL; q = k: known may be NULL; d_out_h of verify and d_h of sign are optional): CC_ERR_DECODE; verify:
 * no request params: CC_ERR_STATE, q != the request params' q: CC_ERR_LEN (sign: q > CC_MAX_Q:
 * CC_ERR_DECODE); k > q: CC_ERR_LEN; n > CC_MAX_BATCH: CC_ERR_DECODE; n = 0: CC_OK, nothing launched.
 * The 2^-4096 event of compute_h giving up is not reported (as cc_sigreq_new_batch_device). */
cc_status cc_sigreq_verify_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* d_commitment,
                                        const uint8_t* d_known, const uint8_t* d_ciphertexts,
                                        const uint8_t* d_elgamal_pk, const uint8_t* d_proofs, const uint8_t* d_chal,
                                        uint8_t* d_verdicts, uint8_t* d_out_h_or_null, void* stream);
cc_status cc_blind_sign_batch_device(cc_ctx* ctx, size_t n, size_t q, size_t k, const uint8_t* d_commitment,
                                     const uint8_t* d_known, const uint8_t* d_ciphertexts, const uint8_t* d_h_or_null,
                                     const uint8_t* x, const uint8_t* y, uint8_t* d_out_h, uint8_t* d_out_c1,
                                     uint8_t* d_out_c2, void* stream);

/* Pedersen VSS share verification (secret_sharing PedersenVSS::verify_share,
 * used by trusted_party_PVSS_keygen, reference keygen.rs:74-122, 334-349), n shares in G1:
 *   g * s + h * s' == sum_{k<t} id^k * C_k, C = commitments[set_of[i]] (n_sets x t x 97 B),
 *   shares n x (s, s') 48 B each, ids n x u64; verdicts n bytes.
 * The keygen derivation alpha_i = g~ * x_i, beta_ij = g~ * y_ij (keygen.rs:17-45) is
 * cc_fixed_base_mul. */
cc_status cc_vss_verify_batch(cc_ctx* ctx, size_t n, size_t t, const uint8_t* g, const uint8_t* h,
                              const uint8_t* commitments, size_t n_sets, const uint32_t* set_of, const uint64_t* ids,
                              const uint8_t* shares, uint8_t* verdicts);

/* Keygen, the dealer's side (reference src/keygen.rs): m independent trusted-party keygens in one call, and
 * the last step of the decentralized keygen.  OG = an OtherGroup encoding.
 *
 * cc_set_keygen_params binds Params.g_tilde (one OG) and the Pedersen generators g, h (G1, 97 B each, as
 * keygen.rs:78-79) and builds the context's own fixed-base window tables: one OtherGroup base for g~ and a
 * two-base G1 table [g, h].  vss_g and vss_h may both be NULL (Shamir only); exactly one NULL, NULL ctx or
 * g_tilde, or table_bits outside {0, 8..16}: CC_ERR_DECODE.  table_bits in 8..16 forces the window width (a
 * width that does not fit the free HBM: CC_ERR_HIP); 0 takes the widest of {16, 13, 12, 10, 8} whose tables
 * fit min(4 GiB, half the free HBM), 8 bits if the allocation fails.  The verkey, issuer and request tables
 * and cc_set_table_bits are untouched.  An identity or undecodable base is skipped in every sum, so its
 * multiples are the identity encoding.  A failed call leaves the context without keygen params.
 *
 * cc_keygen_deal_batch: trusted_party_SSS_keygen (keygen.rs:53-71) or trusted_party_PVSS_keygen (74-122)
 * with keygen_from_shares (17-45), m times; the caller supplies the randomness, the polynomials.
 *   coeffs   m x (q + 1) x t x 48 : polynomial 0 of a keygen shares x, polynomial 1 + j shares y_j;
 *            coefficient i is that of degree i, coefficient 0 the secret
 *   coeffs_t the same layout, the blinding polynomials f' of PedersenVSS::deal; NULL selects Shamir:
 *            out_xt, out_yt and out_comm are then not written and may be NULL
 *   signer ids are 1 .. total, as in the reference
 *   -> out_x  m x total x 48      f_0(id)           out_y  m x total x q x 48   f_{1+j}(id)
 *      out_xt, out_yt             the same shapes, from f'
 *      out_comm m x (q + 1) x t x 97   C_i = f_i g + f'_i h
 *      out_X  m x total x OG      g~ * x_id         out_Y  m x total x q x OG   g~ * y_id,j
 *   The outputs chain without repacking: out_comm is cc_vss_verify_batch's `commitments` with n_sets =
 *   m (q + 1); a keygen's out_X / out_Y slice is cc_set_issuers' X / Y; a signer's x | y is what
 *   cc_blind_sign_batch takes.
 *
 * cc_keygen_combine_batch: the last step of the decentralized keygen (keygen.rs:124-205,
 * PedersenDVSSParticipant::compute_final_comm_coeffs_and_shares [EXT, recalled]).  The inputs are the outputs
 * of a deal with m x d keygens, read as m groups of d dealers; every output is the sum over the dealer axis:
 * shares and blinding shares mod r, commitments as G1 point sums (equal addends double, opposite ones give
 * the identity, an identity or undecodable addend is skipped); out_X / out_Y are g~ times the combined
 * shares.  xt, yt, comm and their outputs may all be NULL; one of them given makes all of them required.
 * [EXT, recalled]: the secret_sharing crate is not on this machine.  The contract is the one
 * setup_signers_for_test (keygen.rs:169-205) relies on: a participant's final share is the sum of every
 * dealer's share for its id, the distributed secret is the sum of the dealers' secrets, and the final
 * coefficient commitments are the dealers' sums.
 *
 * Checks, in this order and before the m = 0 shortcut: NULL context: CC_ERR_DECODE; a NULL buffer the call
 * would read or write with m > 0 (q = 0 is allowed, the y buffers may then be NULL): CC_ERR_DECODE; no
 * keygen params, or coeffs_t / comm given while no g, h are bound: CC_ERR_STATE; t = 0 or t > total:
 * CC_ERR_THRESHOLD (our choice: the crate that would decide is not on this machine); total > CC_MAX_IDS,
 * q > CC_MAX_Q, m total (q + 1) or m (q + 1) t above CC_MAX_BATCH (combine: with m d for m), or d = 0:
 * CC_ERR_DECODE; m = 0: CC_OK, nothing launched.
 * Scalars are reduced mod r, outputs are canonical, a zero share gives the identity encoding; nothing is
 * rejected that the reference would not reject.
 * The *_device forms take device pointers, are asynchronous on `stream` (NULL: the context stream) and
 * take no concurrency slot: they first wait for the slots' batches.  A device set forwards to its first
 * device.
 * Secrets: the host forms copy the coefficients (combine: the dealers' shares) to the device and write the
 * shares there; they overwrite those device copies with zeros before returning (the kernels keep the window
 * digits in registers, there is no digit scratch).  The *_device forms read the caller's buffers in place;
 * they have no scratch of their own. */
cc_status cc_set_keygen_params(cc_ctx* ctx, const uint8_t* g_tilde, const uint8_t* vss_g, const uint8_t* vss_h,
                               int table_bits);
cc_status cc_keygen_deal_batch(cc_ctx* ctx, size_t m, size_t q, size_t t, size_t total, const uint8_t* coeffs,
                               const uint8_t* coeffs_t, uint8_t* out_x, uint8_t* out_y, uint8_t* out_xt,
                               uint8_t* out_yt, uint8_t* out_comm, uint8_t* out_X, uint8_t* out_Y);
cc_status cc_keygen_deal_batch_device(cc_ctx* ctx, size_t m, size_t q, size_t t, size_t total,
                                      const uint8_t* d_coeffs, const uint8_t* d_coeffs_t, uint8_t* d_out_x,
                                      uint8_t* d_out_y, uint8_t* d_out_xt, uint8_t* d_out_yt, uint8_t* d_out_comm,
                                      uint8_t* d_out_X, uint8_t* d_out_Y, void* stream);
cc_status cc_keygen_combine_batch(cc_ctx* ctx, size_t m, size_t d, size_t q, size_t t, size_t total,
                                  const uint8_t* x, const uint8_t* y, const uint8_t* xt, const uint8_t* yt,
                                  const uint8_t* comm, uint8_t* out_x, uint8_t* out_y, uint8_t* out_xt,
                                  uint8_t* out_yt, uint8_t* out_comm, uint8_t* out_X, uint8_t* out_Y);
cc_status cc_keygen_combine_batch_device(cc_ctx* ctx, size_t m, size_t d, size_t q, size_t t, size_t total,
                                         const uint8_t* d_x, const uint8_t* d_y, const uint8_t* d_xt,
                                         const uint8_t* d_yt, const uint8_t* d_comm, uint8_t* d_out_x,
                                         uint8_t* d_out_y, uint8_t* d_out_xt, uint8_t* d_out_yt,
                                         uint8_t* d_out_comm, uint8_t* d_out_X, uint8_t* d_out_Y, void* stream);

/* Pedersen VSS verify_share over commitment SETS (the consumer of the deal and the combine: every
 * participant of the decentralized keygen checks every share it receives, keygen.rs:141-157, 334-349).  g and
 * h are the ones bound by cc_set_keygen_params, with its [g, h] table.  Shares of set j are rows
 * [set_begin[j], set_begin[j + 1]) of ids / shares (set_begin: HOST, n_sets + 1 entries; empty sets allowed)
 * and are checked against commitments[j] (t x 97 B).
 *   cc_vss_verify_sets_device : device buffers; rlc = 0: every verdict is the reference's, and equals
 *                               cc_vss_verify_batch's on the same shares whenever g and h lie in G1 or are
 *                               skipped (for a g or h outside G1 that call's (r - s) g is not -(s g)).  Sets whose decodable points (g and h included) all lie in G1
 *                               take one lane a share: Horner with the 64-bit id as a plain integer over
 *                               the set's commitments, decoded once a set, and two table lookups for
 *                               s g + s' h.  A set holding a decodable point outside G1 is IRREGULAR (the
 *                               reference's verdict there depends on id^k mod r): its rows run through
 *                               cc_vss_verify_batch's kernel unchanged, handed -g, -h and r - s, r - s'.
 *                               rlc != 0: every regular set is first checked as ONE (t + 2)-term MSM,
 *                               sum_k A_k C_k - U g - U' h == O with A_k = sum_i delta_i id_i^k, U = sum
 *                               delta_i s_i, U' = sum delta_i s'_i and the 128-bit delta_i of the RLC batch
 *                               mode keyed by seed32 (HOST, 32 B) and the row index; an accepted set's
 *                               verdicts are 1, a rejected set is re-verified per share, so the verdicts
 *                               are rlc = 0's except that a set holding an invalid share is accepted with
 *                               probability <= 2^-127.  Every set is a check of its own.
 *                               The driver reads one status byte a set to decide what to launch: it
 *                               SYNCHRONISES `stream` once (as cc_verify_batch_locate_device).
 *                               stats4 (HOST, may be NULL): sets, sets the RLC check rejected, irregular
 *                               sets, shares verified per share.
 *   cc_vss_verify_sets        : the same over host buffers, on the context stream; rlc != 0 draws a fresh
 *                               seed.
 *   cc_keygen_verify_shares_batch_device : the same kernels over cc_keygen_deal_batch_device's /
 *                               cc_keygen_combine_batch_device's outputs in place: set (keygen, p) has the
 *                               commitments d_comm + (keygen (q + 1) + p) t 97 and the shares of signers
 *                               1 .. total (p = 0: x / xt, p = 1 + j: y_j / yt_j); verdict index
 *                               (keygen (q + 1) + p) total + signer, which is also the delta's row index.
 * When rlc pays (one MI355X, tools/bench_vss_verify.py, DESIGN.md "Device keygen: verify_share"): with every
 * share valid, rlc = 1 took 0.27x the rate of rlc = 0 at five shares a set (t = 3) and 1.40x at a hundred
 * shares a set (t = 67); the crossing between them was not located.  rlc is for sets of tens of shares and
 * more, not for sets of a handful; a set it rejects costs its per-share check on top.
 * Checks, in this order and before the n = 0 shortcut: NULL context, a NULL buffer the call would read or
 * write with n > 0, NULL set_begin, NULL seed32 with rlc != 0 (device forms): CC_ERR_DECODE; no keygen
 * params or no g, h bound: CC_ERR_STATE; t = 0 or t > 4096, n, n_sets or n_sets t above CC_MAX_BATCH,
 * set_begin[0] != 0, set_begin[n_sets] != n, set_begin decreasing somewhere: CC_ERR_DECODE; the keygen-shaped
 * call: t > total: CC_ERR_THRESHOLD (as the deal), then total > CC_MAX_IDS, q > CC_MAX_Q or a size above
 * CC_MAX_BATCH: CC_ERR_DECODE; n = 0: CC_OK, nothing launched.
 * Nothing is rejected that the reference would not reject: scalars are reduced mod r, a commitment that
 * does not decode is the identity and is skipped, an identity or undecodable g or h is skipped in every sum.
 * The calls take no concurrency slot: they first wait for the slots' batches and are ordered on the
 * context's stream.  A device set forwards to its first device. */
cc_status cc_vss_verify_sets_device(cc_ctx* ctx, size_t n, size_t t, size_t n_sets, const uint64_t* set_begin,
                                    const uint8_t* d_commitments, const uint64_t* d_ids, const uint8_t* d_shares,
                                    int rlc, const uint8_t* seed32, uint8_t* d_verdicts, uint32_t* stats4_or_null,
                                    void* stream);
cc_status cc_vss_verify_sets(cc_ctx* ctx, size_t n, size_t t, size_t n_sets, const uint64_t* set_begin,
                             const uint8_t* commitments, const uint64_t* ids, const uint8_t* shares, int rlc,
                             uint8_t* verdicts, uint32_t* stats4_or_null);
cc_status cc_keygen_verify_shares_batch_device(cc_ctx* ctx, size_t m, size_t q, size_t t, size_t total,
                                               const uint8_t* d_x, const uint8_t* d_y, const uint8_t* d_xt,
                                               const uint8_t* d_yt, const uint8_t* d_comm, int rlc,
                                               const uint8_t* seed32, uint8_t* d_verdicts, uint32_t* stats4_or_null,
                                               void* stream);

/* Batch fixed-base scalar multiplication out_i = k_i * base (group 1 = G1, 2 = G2); scalars n x 48 B
 * big-endian Fr, out n encodings.  The keygen derivation g~ * x_i (reference src/keygen.rs:27-32)
 * and the issuer's h^e (src/signature.rs:423-428) in batch form. */
cc_status cc_fixed_base_mul(cc_ctx* ctx, int group, const uint8_t* base, size_t n, const uint8_t* scalars,
                            uint8_t* out);

/* Kernel timing of the last cc_verify_batch_device call (HIP events on the context stream):
 * milliseconds per phase {prep, miller, fexp}.  Used by bench.py for the roofline figure. */
cc_status cc_last_timing(const cc_ctx* ctx, float* prep_ms, float* miller_ms, float* fexp_ms);
cc_status cc_set_timing(cc_ctx* ctx, int enabled);

/* Device self-test of the lazy radix-2^28 field core the pairing kernels use (csrc/lazy.h): op 0
 * (a b + c d) / 2^392, op 1 a b / 2^392 (signed product scanning with Montgomery reduction), op 2 the
 * value reduction, op 3 the limb squeeze, op 6 the canonical residue (12 words in columns 0..11), on n
 * elements of 14 signed 28-bit-radix limbs (host arrays, n x 14 int32; b, c, d may be NULL for ops
 * 1-3 and 6; ops 4 and 5: the divstep inversions).  Test infrastructure: the tests drive it
 * at the limits of the compile-time bounds and compare with big-integer arithmetic.  Returns 0, or
 * -1 on a HIP error or an unknown op.  No context needed (current device). */
int cc_selftest_lazy(int op, size_t n, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d,
                     int32_t* out);

/* Device self-test of the canonical 12 x 32 Fp every non-pairing kernel uses (csrc/field.h, with the
 * out-of-line product), of its Fp2 helpers and of the scalar field (csrc/fr.h, csrc/codec.h), one row
 * per lane on n rows of 12 words (host arrays; unused high words zero; b may be NULL for a one-operand
 * op).  Fp ops, raw rows in and out: 0 fp_add, 1 fp_sub, 2 fp_neg, 3 fp_dbl, 4 fp_mul and 5 fp_sqr
 * (a b / 2^406 mod p on the rows as given), 6 fp_to_mont, 7 fp_from_mont, 8 fp_raw_reduce (a < 2^384),
 * 9 fp_inv (Montgomery form in and out).  Fp2 ops, row i of a the real and row i of b the imaginary
 * half of one operand, out holding 2n rows (real halves, then imaginary halves): 10 f2_mul (by row
 * (i + 1) mod n), 11 f2_sqr, 12 f2_inv, 13 f2_mul_xi.  Fr ops on words 0..7: 14 fm_mul_v, 15 fm_sub,
 * 16 fm_reduce_once (a = a raw sum below 2r), 17 fm_from_u64 (words 0..1), 18 fm_to_canon,
 * 19 fr_mul_canon, 20 fr_inv_int, 21 fm_inv, 22 rlc_delta_abs (magnitude in words 0..7, sign in word
 * 8), 23 fr_from_be48 (the row read as 48 big-endian bytes).  Test infrastructure, as above.  Returns 0,
 * or -1 on a HIP error or an unknown op. */
int cc_selftest_field(int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out);

#ifdef __cplusplus
}
#endif

#endif /* COCONUT_HIP_H */
