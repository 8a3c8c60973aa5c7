// src/batch.rs — batch entry points on the reference crate's own types (src/signature.rs), through
// src/hip.rs.  Encodings are exactly amcl_wrapper's to_bytes() (G1 97 B, G2 192 B, Fr 48 B), so the
// glue only concatenates.  Where the reference panics the shim panics too (HipCtx::check).
// Every wrapper asserts, before its unsafe call, each length the C side derives its reads from
// (`len-guard` lines; tests/test_rust_binding.py checks they are present): the C ABI reads n * q * 48
// bytes of messages, n * len entries of a batch, ..., so a shorter Vec would be a heap over-read.
use crate::hip::*;
use crate::keygen::Signer;
use crate::signature::{BlindSignature, Params, Signature, SignatureRequest, Sigkey, Verkey};
use crate::{OtherGroup, SignatureGroup};
use amcl_wrapper::field_elem::FieldElement;
use amcl_wrapper::group_elem::GroupElement;
use amcl_wrapper::group_elem_g1::G1;
use std::os::raw::c_int;

/// Smallest batch routed to the GPU.  One `Signature::verify` costs ~2.1 ms through the engine (its
/// one-wave kernels' dependency chains) against ~1.9 ms for the reference's own CPU
/// path on one host thread; two credentials already take ~3.7 ms on the CPU and still ~2.1 ms on the
/// GPU.  So a single credential keeps the reference path and only batches go to the device.
pub const GPU_MIN_BATCH: usize = 2;

impl Signature {
    /// Batch form of `Signature::verify` (signature.rs:473-478): one verkey for the whole batch.
    /// Below GPU_MIN_BATCH credentials it is the reference's own verify, unchanged.
    pub fn verify_batch(sigs: &[Signature], messages: &[Vec<FieldElement>], vk: &Verkey,
                        params: &Params, ctx: &HipCtx) -> Vec<bool> {
        let q = vk.Y_tilde.len();
        assert_eq!(messages.len(), sigs.len(), "one message vector per signature");  // len-guard
        assert!(messages.iter().all(|m| m.len() == q), "Verkey valid for {} messages", q);  // len-guard
        if sigs.len() < GPU_MIN_BATCH {
            return sigs.iter().zip(messages).map(|(s, m)| s.verify(m, vk, params)).collect();
        }
        let s1: Vec<u8> = sigs.iter().flat_map(|s| s.sigma_1.to_bytes()).collect();
        let s2: Vec<u8> = sigs.iter().flat_map(|s| s.sigma_2.to_bytes()).collect();
        let m:  Vec<u8> = messages.iter().flatten().flat_map(|f| f.to_bytes()).collect();
        ctx.set_params(&params.g_tilde.to_bytes());
        ctx.set_verkey(&vk.X_tilde.to_bytes(),
                       &vk.Y_tilde.iter().flat_map(|y| y.to_bytes()).collect::<Vec<u8>>(), q);
        let mut verdicts = vec![0u8; sigs.len()];
        let st = unsafe { cc_verify_batch(ctx.raw, sigs.len(), q, s1.as_ptr(), s2.as_ptr(), m.as_ptr(),
                                          std::ptr::null(), std::ptr::null(), verdicts.as_mut_ptr(),
                                          std::ptr::null_mut(), 0) };
        assert_eq!(st, 0, "{}", ctx.status_str(st));
        verdicts.into_iter().map(|v| v == 1).collect()
    }

    /// Batch form of `Signature::aggregate` (signature.rs:448-470).
    pub fn aggregate_batch(threshold: usize, batches: &[Vec<(usize, Signature)>], ctx: &HipCtx) -> Vec<Signature> {
        if batches.is_empty() { return Vec::new(); }
        let len = batches[0].len();
        assert!(batches.iter().all(|b| b.len() == len), "every batch has the same length");  // len-guard
        assert!(len >= threshold);                                   // signature.rs:449
        let ids: Vec<u64> = batches.iter().flatten().map(|(i, _)| *i as u64).collect();
        let s1: Vec<u8> = batches.iter().flatten().flat_map(|(_, s)| s.sigma_1.to_bytes()).collect();
        let s2: Vec<u8> = batches.iter().flatten().flat_map(|(_, s)| s.sigma_2.to_bytes()).collect();
        let sb = ctx.sig_bytes();
        assert!(s1.len() == ids.len() * sb && s2.len() == ids.len() * sb, "signature encodings");  // len-guard
        let (mut o1, mut o2) = (vec![0u8; sb * batches.len()], vec![0u8; sb * batches.len()]);
        let st = unsafe { cc_signature_aggregate_batch(ctx.raw, batches.len(), len, threshold, ids.as_ptr(),
                                                       s1.as_ptr(), s2.as_ptr(), o1.as_mut_ptr(), o2.as_mut_ptr()) };
        assert_eq!(st, 0, "{}", ctx.status_str(st));
        o1.chunks(sb).zip(o2.chunks(sb)).map(|(a, b)| Signature {
            sigma_1: SignatureGroup::from_bytes(a).unwrap(), sigma_2: SignatureGroup::from_bytes(b).unwrap() }).collect()
    }
}

fn pack(msgs: &[Vec<u8>]) -> (Vec<u8>, Vec<u64>) {
    let mut offs = vec![0u64];
    let mut data = Vec::new();
    for m in msgs { data.extend_from_slice(m); offs.push(data.len() as u64); }
    (data, offs)
}

impl Params {
    /// Params::new (signature.rs:22-32) with every from_msg_hash on the GPU, one call per group.
    pub fn new_hip(msg_count: usize, label: &[u8], ctx: &HipCtx) -> Params {
        let (sg, og) = if ctx.mode() == CC_SIG_G2 { (2, 1) } else { (1, 2) };
        let eb = |g: c_int| if g == 1 { 97 } else { 192 };
        let mut sig_msgs = vec![[label, b" : g"].concat()];
        for i in 0..msg_count { sig_msgs.push([label, format!(" : y{}", i).as_bytes()].concat()); }
        let (data, offs) = pack(&sig_msgs);
        let mut sig = vec![0u8; sig_msgs.len() * eb(sg)];
        ctx.check(unsafe { cc_hash_to_curve(ctx.raw, sg, sig_msgs.len(), data.as_ptr(), offs.as_ptr(), sig.as_mut_ptr()) });
        let (data, offs) = pack(&[[label, b" : g_tilde"].concat()]);
        let mut gt = vec![0u8; eb(og)];
        ctx.check(unsafe { cc_hash_to_curve(ctx.raw, og, 1, data.as_ptr(), offs.as_ptr(), gt.as_mut_ptr()) });
        let chunks: Vec<&[u8]> = sig.chunks(eb(sg)).collect();
        Params { g: SignatureGroup::from_bytes(chunks[0]).unwrap(),
                 g_tilde: OtherGroup::from_bytes(&gt).unwrap(),
                 h: chunks[1..].iter().map(|c| SignatureGroup::from_bytes(c).unwrap()).collect() }
    }
}

impl BlindSignature {
    /// BlindSignature::new (signature.rs:382-433) for n requests under one Sigkey; every request
    /// has k hidden and q - k known messages.
    pub fn new_batch(reqs: &[SignatureRequest], sigkey: &Sigkey, ctx: &HipCtx) -> Vec<BlindSignature> {
        let (n, q) = (reqs.len(), sigkey.y.len());
        if n == 0 { return Vec::new(); }
        let k = reqs[0].ciphertexts.len();
        assert!(k <= q && reqs.iter().all(|r| r.ciphertexts.len() == k && r.known_messages.len() == q - k),
                "every request has k hidden and q - k known messages");  // len-guard
        let cm: Vec<u8> = reqs.iter().flat_map(|r| r.commitment.to_bytes()).collect();
        let kn: Vec<u8> = reqs.iter().flat_map(|r| r.known_messages.iter().flat_map(|m| m.to_bytes())).collect();
        let ct: Vec<u8> = reqs.iter().flat_map(|r| r.ciphertexts.iter()
                              .flat_map(|c| [c.0.to_bytes(), c.1.to_bytes()].concat())).collect();
        let y: Vec<u8> = sigkey.y.iter().flat_map(|v| v.to_bytes()).collect();
        let sb = ctx.sig_bytes();
        assert_eq!(cm.len(), n * sb, "commitment encodings");  // len-guard
        let (mut h, mut c1, mut c2) = (vec![0u8; n * sb], vec![0u8; n * sb], vec![0u8; n * sb]);
        ctx.check(unsafe { cc_blind_sign_batch(ctx.raw, n, q, k, cm.as_ptr(), kn.as_ptr(), ct.as_ptr(),
                                               sigkey.x.to_bytes().as_ptr(), y.as_ptr(),
                                               h.as_mut_ptr(), c1.as_mut_ptr(), c2.as_mut_ptr()) });
        (0..n).map(|i| BlindSignature {
            h: SignatureGroup::from_bytes(&h[i * sb..(i + 1) * sb]).unwrap(),
            blinded: (SignatureGroup::from_bytes(&c1[i * sb..(i + 1) * sb]).unwrap(),
                      SignatureGroup::from_bytes(&c2[i * sb..(i + 1) * sb]).unwrap()) }).collect()
    }
}

/// PedersenVSS::verify_share (keygen.rs:332-351) for n shares; share i is checked against
/// commitment set set_of[i] (each set t x G1 bytes).
pub fn verify_shares_batch(t: usize, g: &G1, h: &G1, sets: &[Vec<G1>], set_of: &[u32], ids: &[u64],
                           shares: &[(FieldElement, FieldElement)], ctx: &HipCtx) -> Vec<bool> {
    assert!(set_of.len() == ids.len() && shares.len() == ids.len(), "one set, id and share per check");  // len-guard
    assert!(sets.iter().all(|s| s.len() == t), "every commitment set has t points");  // len-guard
    assert!(set_of.iter().all(|&k| (k as usize) < sets.len()), "set index in range");  // len-guard
    let cm: Vec<u8> = sets.iter().flatten().flat_map(|c| c.to_bytes()).collect();
    let sh: Vec<u8> = shares.iter().flat_map(|(s, st)| [s.to_bytes(), st.to_bytes()].concat()).collect();
    let mut v = vec![0u8; ids.len()];
    ctx.check(unsafe { cc_vss_verify_batch(ctx.raw, ids.len(), t, g.to_bytes().as_ptr(), h.to_bytes().as_ptr(),
                                           cm.as_ptr(), sets.len(), set_of.as_ptr(), ids.as_ptr(), sh.as_ptr(),
                                           v.as_mut_ptr()) });
    v.into_iter().map(|b| b == 1).collect()
}

/// PedersenVSS::verify_share for the shares of whole commitment sets under the g, h bound by
/// cc_set_keygen_params: shares[j] are the (id, s, s') received for sets[j].  rlc: one random-linear-combination
/// check a set first, per share only where it fails.  One Vec<bool> per set.
pub fn verify_share_sets_batch(t: usize, sets: &[Vec<G1>], shares: &[Vec<(u64, FieldElement, FieldElement)>],
                               rlc: bool, ctx: &HipCtx) -> Vec<Vec<bool>> {
    assert!(shares.len() == sets.len(), "one share list per commitment set");  // len-guard
    assert!(sets.iter().all(|s| s.len() == t), "every commitment set has t points");  // len-guard
    let mut set_begin: Vec<u64> = vec![0];
    for s in shares { set_begin.push(set_begin[set_begin.len() - 1] + s.len() as u64); }
    let n = set_begin[sets.len()] as usize;
    let cm: Vec<u8> = sets.iter().flatten().flat_map(|c| c.to_bytes()).collect();
    let ids: Vec<u64> = shares.iter().flatten().map(|s| s.0).collect();
    let sh: Vec<u8> = shares.iter().flatten().flat_map(|(_, s, st)| [s.to_bytes(), st.to_bytes()].concat()).collect();
    assert!(cm.len() == sets.len() * t * 97 && sh.len() == n * 96, "encodings");  // len-guard
    let mut v = vec![0u8; n];
    ctx.check(unsafe { cc_vss_verify_sets(ctx.raw, n, t, sets.len(), set_begin.as_ptr(), cm.as_ptr(), ids.as_ptr(),
                                          sh.as_ptr(), rlc as c_int, v.as_mut_ptr(), std::ptr::null_mut()) });
    (0..sets.len()).map(|j| v[set_begin[j] as usize..set_begin[j + 1] as usize].iter().map(|&b| b == 1).collect())
        .collect()
}

impl Verkey {
    /// Batch form of `Verkey::aggregate` (signature.rs:483-526): n aggregations of `len` (id, Verkey)
    /// entries each; only the first `threshold` are used (HashSet semantics of the ids as there).
    pub fn aggregate_batch(threshold: usize, batches: &[Vec<(usize, &Verkey)>], ctx: &HipCtx) -> Vec<Verkey> {
        if batches.is_empty() { return Vec::new(); }
        let (n, len) = (batches.len(), batches[0].len());
        assert!(batches.iter().all(|b| b.len() == len), "every batch has the same length");  // len-guard
        assert!(len >= threshold);                                   // signature.rs:484
        let q = batches[0][0].1.Y_tilde.len();
        assert!(batches.iter().flatten().all(|(_, vk)| vk.Y_tilde.len() == q));  // signature.rs:486-488
        let ids: Vec<u64> = batches.iter().flatten().map(|(i, _)| *i as u64).collect();
        let x: Vec<u8> = batches.iter().flatten().flat_map(|(_, vk)| vk.X_tilde.to_bytes()).collect();
        let y: Vec<u8> = batches.iter().flatten()
            .flat_map(|(_, vk)| vk.Y_tilde.iter().flat_map(|v| v.to_bytes())).collect();
        let ob = ctx.oth_bytes();
        assert!(x.len() == ids.len() * ob && y.len() == ids.len() * q * ob, "verkey encodings");  // len-guard
        let (mut ox, mut oy) = (vec![0u8; n * ob], vec![0u8; n * q * ob]);
        ctx.check(unsafe { cc_verkey_aggregate_batch(ctx.raw, n, len, threshold, q, ids.as_ptr(), x.as_ptr(),
                                                     y.as_ptr(), ox.as_mut_ptr(), oy.as_mut_ptr()) });
        (0..n).map(|i| Verkey {
            X_tilde: OtherGroup::from_bytes(&ox[i * ob..(i + 1) * ob]).unwrap(),
            Y_tilde: (0..q).map(|j| OtherGroup::from_bytes(&oy[(i * q + j) * ob..(i * q + j + 1) * ob]).unwrap())
                .collect::<Vec<OtherGroup>>().into() }).collect()
    }
}

/// PoKOfSignatureProof::verify (ps_sig, called at pok_sig.rs:103-105) for n proofs against one verkey:
/// each proof as its serialized parts (sigma'_1, sigma'_2, J, Schnorr commitment T, responses ordered
/// [g~, Y~_i for hidden i ascending] as ps_sig builds them), one challenge and the revealed messages
/// (indices shared by the batch, ascending).  CC_ERR_BASES_EXPS -> ps_sig's UnequalNoOfBasesExponents.
pub fn pok_verify_batch(proofs: &[(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<FieldElement>)], chal: &[FieldElement],
                        revealed_idx: &[u64], revealed_msgs: &[Vec<FieldElement>], vk: &Verkey, params: &Params,
                        ctx: &HipCtx) -> Vec<bool> {
    let (n, q, r) = (proofs.len(), vk.Y_tilde.len(), revealed_idx.len());
    if n == 0 { return Vec::new(); }
    let nresp = proofs[0].4.len();
    let (sb, ob) = (ctx.sig_bytes(), ctx.oth_bytes());
    assert_eq!(chal.len(), n, "one challenge per proof");  // len-guard
    assert!(revealed_msgs.len() == n && revealed_msgs.iter().all(|m| m.len() == r),
            "r revealed messages per proof");  // len-guard
    assert!(proofs.iter().all(|p| p.4.len() == nresp), "the same response count for every proof");  // len-guard
    assert!(proofs.iter().all(|p| p.0.len() == sb && p.1.len() == sb && p.2.len() == ob && p.3.len() == ob),
            "proof part encodings (sigma'_1, sigma'_2: SignatureGroup; J, T: OtherGroup)");  // len-guard
    ctx.set_params(&params.g_tilde.to_bytes());
    ctx.set_verkey(&vk.X_tilde.to_bytes(), &vk.Y_tilde.iter().flat_map(|y| y.to_bytes()).collect::<Vec<u8>>(), q);
    let cat = |f: &dyn Fn(&(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<FieldElement>)) -> Vec<u8>| -> Vec<u8> {
        proofs.iter().flat_map(|p| f(p)).collect()
    };
    let (s1, s2, j, t) = (cat(&|p| p.0.clone()), cat(&|p| p.1.clone()), cat(&|p| p.2.clone()), cat(&|p| p.3.clone()));
    let resp = cat(&|p| p.4.iter().flat_map(|v| v.to_bytes()).collect());
    let ch: Vec<u8> = chal.iter().flat_map(|c| c.to_bytes()).collect();
    let rm: Vec<u8> = revealed_msgs.iter().flatten().flat_map(|m| m.to_bytes()).collect();
    let mut v = vec![0u8; n];
    ctx.check(unsafe { cc_pok_verify_batch(ctx.raw, n, q, r, nresp, s1.as_ptr(), s2.as_ptr(), j.as_ptr(), t.as_ptr(),
                                           resp.as_ptr(), ch.as_ptr(), revealed_idx.as_ptr(), rm.as_ptr(),
                                           v.as_mut_ptr(), std::ptr::null_mut()) });
    v.into_iter().map(|b| b == 1).collect()
}

/// PoKOfSignatureProof::verify for n proofs, proof i against ITS OWN verkey `vks[i]` (a verifier whose
/// credentials come from different authority subsets holds one aggregated verkey per credential).  The
/// other arguments as `pok_verify_batch`; revealed indices may be in any order.  Binds params only.
pub fn pok_verify_batch_pervk(proofs: &[(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<FieldElement>)],
                              chal: &[FieldElement], revealed_idx: &[u64], revealed_msgs: &[Vec<FieldElement>],
                              vks: &[Verkey], params: &Params, ctx: &HipCtx) -> Vec<bool> {
    let (n, r) = (proofs.len(), revealed_idx.len());
    if n == 0 { return Vec::new(); }
    assert_eq!(vks.len(), n, "one verkey per proof");  // len-guard
    let q = vks[0].Y_tilde.len();
    let nresp = proofs[0].4.len();
    let (sb, ob) = (ctx.sig_bytes(), ctx.oth_bytes());
    assert!(vks.iter().all(|v| v.Y_tilde.len() == q), "the same message count for every verkey");  // len-guard
    assert_eq!(chal.len(), n, "one challenge per proof");  // len-guard
    assert!(revealed_msgs.len() == n && revealed_msgs.iter().all(|m| m.len() == r),
            "r revealed messages per proof");  // len-guard
    assert!(proofs.iter().all(|p| p.4.len() == nresp), "the same response count for every proof");  // len-guard
    assert!(proofs.iter().all(|p| p.0.len() == sb && p.1.len() == sb && p.2.len() == ob && p.3.len() == ob),
            "proof part encodings (sigma'_1, sigma'_2: SignatureGroup; J, T: OtherGroup)");  // len-guard
    ctx.set_params(&params.g_tilde.to_bytes());
    let cat = |f: &dyn Fn(&(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<FieldElement>)) -> Vec<u8>| -> Vec<u8> {
        proofs.iter().flat_map(|p| f(p)).collect()
    };
    let (s1, s2, j, t) = (cat(&|p| p.0.clone()), cat(&|p| p.1.clone()), cat(&|p| p.2.clone()), cat(&|p| p.3.clone()));
    let resp = cat(&|p| p.4.iter().flat_map(|v| v.to_bytes()).collect());
    let ch: Vec<u8> = chal.iter().flat_map(|c| c.to_bytes()).collect();
    let rm: Vec<u8> = revealed_msgs.iter().flatten().flat_map(|m| m.to_bytes()).collect();
    let vx: Vec<u8> = vks.iter().flat_map(|v| v.X_tilde.to_bytes()).collect();
    let vy: Vec<u8> = vks.iter().flat_map(|v| v.Y_tilde.iter().flat_map(|y| y.to_bytes())).collect();
    assert!(vx.len() == n * ob && vy.len() == n * q * ob, "verkey encodings (OtherGroup)");  // len-guard
    let mut v = vec![0u8; n];
    ctx.check(unsafe { cc_pok_verify_batch_pervk(ctx.raw, n, q, r, nresp, s1.as_ptr(), s2.as_ptr(), j.as_ptr(),
                                                 t.as_ptr(), resp.as_ptr(), ch.as_ptr(), revealed_idx.as_ptr(),
                                                 rm.as_ptr(), vx.as_ptr(), vy.as_ptr(), v.as_mut_ptr(),
                                                 std::ptr::null_mut()) });
    v.into_iter().map(|b| b == 1).collect()
}

/// `pok_verify_batch` through the RLC locate mode (cc_pok_verify_batch_locate): the batch is checked in
/// segments of `seg` proofs (a power of two >= 4; 0: the engine's default for the group mode), each with its
/// own random-linear-combination check, and only the rejected segments are verified per proof, so a forged
/// showing costs its segment's re-verification, not the batch's.  The verdicts equal `pok_verify_batch`'s;
/// the second value is (segments, rejected segments, proofs rechecked).
pub fn pok_verify_batch_locate(proofs: &[(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<FieldElement>)],
                               chal: &[FieldElement], revealed_idx: &[u64], revealed_msgs: &[Vec<FieldElement>],
                               vk: &Verkey, params: &Params, seg: usize, ctx: &HipCtx) -> (Vec<bool>, [u32; 3]) {
    let (n, q, r) = (proofs.len(), vk.Y_tilde.len(), revealed_idx.len());
    if n == 0 { return (Vec::new(), [0; 3]); }
    let nresp = proofs[0].4.len();
    let (sb, ob) = (ctx.sig_bytes(), ctx.oth_bytes());
    assert_eq!(chal.len(), n, "one challenge per proof");  // len-guard
    assert!(revealed_msgs.len() == n && revealed_msgs.iter().all(|m| m.len() == r),
            "r revealed messages per proof");  // len-guard
    assert!(proofs.iter().all(|p| p.4.len() == nresp), "the same response count for every proof");  // len-guard
    assert!(proofs.iter().all(|p| p.0.len() == sb && p.1.len() == sb && p.2.len() == ob && p.3.len() == ob),
            "proof part encodings (sigma'_1, sigma'_2: SignatureGroup; J, T: OtherGroup)");  // len-guard
    ctx.set_params(&params.g_tilde.to_bytes());
    ctx.set_verkey(&vk.X_tilde.to_bytes(), &vk.Y_tilde.iter().flat_map(|y| y.to_bytes()).collect::<Vec<u8>>(), q);
    let cat = |f: &dyn Fn(&(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<FieldElement>)) -> Vec<u8>| -> Vec<u8> {
        proofs.iter().flat_map(|p| f(p)).collect()
    };
    let (s1, s2, j, t) = (cat(&|p| p.0.clone()), cat(&|p| p.1.clone()), cat(&|p| p.2.clone()), cat(&|p| p.3.clone()));
    let resp = cat(&|p| p.4.iter().flat_map(|v| v.to_bytes()).collect());
    let ch: Vec<u8> = chal.iter().flat_map(|c| c.to_bytes()).collect();
    let rm: Vec<u8> = revealed_msgs.iter().flatten().flat_map(|m| m.to_bytes()).collect();
    let mut v = vec![0u8; n];
    let mut stats = [0u32; 3];
    ctx.check(unsafe { cc_pok_verify_batch_locate(ctx.raw, n, q, r, nresp, seg, s1.as_ptr(), s2.as_ptr(), j.as_ptr(),
                                                  t.as_ptr(), resp.as_ptr(), ch.as_ptr(), revealed_idx.as_ptr(),
                                                  rm.as_ptr(), v.as_mut_ptr(), stats.as_mut_ptr()) });
    (v.into_iter().map(|b| b == 1).collect(), stats)
}

/// One holder-side proof as its serialized parts: (sigma'_1, sigma'_2, J, T, responses), the tuple
/// `pok_verify_batch` takes.
pub type ProofParts = (Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<FieldElement>);

/// PoKOfSignature::init + gen_proof (ps_sig, called at pok_sig.rs:80-100) for n credentials under one
/// verkey: fresh r1, r2 and blindings per credential (FieldElement::random), both sigma' and J, T on the
/// GPU, the challenge as the reference derives it (pok_sig.rs:94: from_msg_hash of to_bytes), the
/// responses on the GPU.  Returns every proof's parts and its challenge.
pub fn pok_prove_batch(sigs: &[Signature], messages: &[Vec<FieldElement>], revealed_idx: &[u64], vk: &Verkey,
                       params: &Params, ctx: &HipCtx) -> Vec<(ProofParts, FieldElement)> {
    let (n, q, r) = (sigs.len(), vk.Y_tilde.len(), revealed_idx.len());
    if n == 0 { return Vec::new(); }
    assert_eq!(messages.len(), n, "one message vector per signature");  // len-guard
    assert!(messages.iter().all(|m| m.len() == q), "Verkey valid for {} messages", q);  // len-guard
    assert!(r <= q && revealed_idx.iter().all(|&i| (i as usize) < q), "revealed indices below q");  // len-guard
    let nresp = q - r + 1;
    let (sb, ob) = (ctx.sig_bytes(), ctx.oth_bytes());
    let s1: Vec<u8> = sigs.iter().flat_map(|s| s.sigma_1.to_bytes()).collect();
    let s2: Vec<u8> = sigs.iter().flat_map(|s| s.sigma_2.to_bytes()).collect();
    let m: Vec<u8> = messages.iter().flatten().flat_map(|f| f.to_bytes()).collect();
    let rand: Vec<u8> = (0..n * (nresp + 2)).flat_map(|_| FieldElement::random().to_bytes()).collect();
    assert!(s1.len() == n * sb && s2.len() == n * sb, "signature encodings");  // len-guard
    assert!(m.len() == n * q * 48 && rand.len() == n * (nresp + 2) * 48, "scalar encodings");  // len-guard
    ctx.set_params(&params.g_tilde.to_bytes());
    ctx.set_verkey(&vk.X_tilde.to_bytes(), &vk.Y_tilde.iter().flat_map(|y| y.to_bytes()).collect::<Vec<u8>>(), q);
    let (mut o1, mut o2) = (vec![0u8; n * sb], vec![0u8; n * sb]);
    let (mut oj, mut ot) = (vec![0u8; n * ob], vec![0u8; n * ob]);
    ctx.check(unsafe { cc_pok_init_batch(ctx.raw, n, q, r, nresp, s1.as_ptr(), s2.as_ptr(), m.as_ptr(),
                                         revealed_idx.as_ptr(), rand.as_ptr(), o1.as_mut_ptr(), o2.as_mut_ptr(),
                                         oj.as_mut_ptr(), ot.as_mut_ptr()) });
    // to_bytes: sigma'_1 || sigma'_2 || J || g~ || Y~_hidden.. || T
    let mut bases = params.g_tilde.to_bytes();
    for i in 0..q {
        if !revealed_idx.contains(&(i as u64)) { bases.extend_from_slice(&vk.Y_tilde[i].to_bytes()); }
    }
    let chals: Vec<FieldElement> = (0..n).map(|i| {
        let row = [&o1[i * sb..(i + 1) * sb], &o2[i * sb..(i + 1) * sb], &oj[i * ob..(i + 1) * ob], &bases[..],
                   &ot[i * ob..(i + 1) * ob]].concat();
        FieldElement::from_msg_hash(&row)
    }).collect();
    let ch: Vec<u8> = chals.iter().flat_map(|c| c.to_bytes()).collect();
    assert_eq!(ch.len(), n * 48, "challenge encodings");  // len-guard
    let mut resp = vec![0u8; n * nresp * 48];
    ctx.check(unsafe { cc_pok_gen_proof_batch(ctx.raw, n, q, r, nresp, m.as_ptr(), revealed_idx.as_ptr(),
                                              rand.as_ptr(), ch.as_ptr(), resp.as_mut_ptr()) });
    chals.into_iter().enumerate().map(|(i, c)| {
        let rs = (0..nresp).map(|k| FieldElement::from_bytes(&resp[(i * nresp + k) * 48..(i * nresp + k + 1) * 48]).unwrap())
            .collect();
        ((o1[i * sb..(i + 1) * sb].to_vec(), o2[i * sb..(i + 1) * sb].to_vec(), oj[i * ob..(i + 1) * ob].to_vec(),
          ot[i * ob..(i + 1) * ob].to_vec(), rs), c)
    }).collect()
}

/// BlindSignature::unblind (signature.rs:436-443) for n blind signatures, each with its own ElGamal
/// secret key: Signature { sigma_1: h, sigma_2: c~2 - sk c~1 }.
pub fn unblind_batch(blind: &[BlindSignature], sks: &[FieldElement], ctx: &HipCtx) -> Vec<Signature> {
    let n = blind.len();
    if n == 0 { return Vec::new(); }
    assert_eq!(sks.len(), n, "one ElGamal secret key per blind signature");  // len-guard
    let sb = ctx.sig_bytes();
    let c1: Vec<u8> = blind.iter().flat_map(|b| b.blinded.0.to_bytes()).collect();
    let c2: Vec<u8> = blind.iter().flat_map(|b| b.blinded.1.to_bytes()).collect();
    let sk: Vec<u8> = sks.iter().flat_map(|s| s.to_bytes()).collect();
    assert!(c1.len() == n * sb && c2.len() == n * sb && sk.len() == n * 48, "ciphertext and key encodings");  // len-guard
    let mut out = vec![0u8; n * sb];
    ctx.check(unsafe { cc_unblind_batch(ctx.raw, n, c1.as_ptr(), c2.as_ptr(), sk.as_ptr(), out.as_mut_ptr()) });
    blind.iter().enumerate().map(|(i, b)| Signature {
        sigma_1: b.h.clone(), sigma_2: SignatureGroup::from_bytes(&out[i * sb..(i + 1) * sb]).unwrap() }).collect()
}

/// One prepared signature request: the request itself, the randomness `SignatureRequest::new` returns
/// (r, k_0 ..), the serialized SignatureRequestProof record `cc_sigreq_verify_batch` reads, and its
/// challenge.
pub type PreparedRequest = (SignatureRequest, Vec<FieldElement>, Vec<u8>, FieldElement);

/// SignatureRequest::new + SignatureRequestPoK::init / gen_proof (signature.rs:124-320) for n holders,
/// each hiding the first k of its q messages under its own ElGamal key: fresh r, k_i and blindings per
/// request (FieldElement::random), every commitment, ciphertext and Schnorr commitment on the GPU, the
/// challenge as the reference derives it (from_msg_hash of SignatureRequestPoK::to_bytes), the responses
/// on the GPU.
pub fn sigreq_prove_batch(messages: &[Vec<FieldElement>], k: usize, elgamal_pks: &[SignatureGroup],
                          elgamal_sks: &[FieldElement], params: &Params, ctx: &HipCtx) -> Vec<PreparedRequest> {
    let (n, q) = (messages.len(), params.h.len());
    if n == 0 { return Vec::new(); }
    let sb = ctx.sig_bytes();
    let gb = params.g.to_bytes();
    let hb: Vec<u8> = params.h.iter().flat_map(|p| p.to_bytes()).collect();
    assert_eq!(params.h.len(), q, "one h per message");  // len-guard
    assert!(q > 0 && k <= q, "k hidden of q messages");  // len-guard
    assert!(gb.len() == sb && hb.len() == q * sb, "params encodings");  // len-guard
    ctx.check(unsafe { cc_set_request_params(ctx.raw, q, gb.as_ptr(), hb.as_ptr(), 0) });
    assert!(messages.iter().all(|m| m.len() == q), "Params valid for {} messages", q);  // len-guard
    assert_eq!(elgamal_pks.len(), n, "one ElGamal public key per request");  // len-guard
    assert_eq!(elgamal_sks.len(), n, "one ElGamal secret key per request");  // len-guard
    let pb = unsafe { cc_sigreq_proof_bytes(ctx.raw, k) };
    let m: Vec<u8> = messages.iter().flatten().flat_map(|f| f.to_bytes()).collect();
    let pk: Vec<u8> = elgamal_pks.iter().flat_map(|p| p.to_bytes()).collect();
    let rand: Vec<u8> = (0..n * (k + 1)).flat_map(|_| FieldElement::random().to_bytes()).collect();
    assert!(m.len() == n * q * 48 && pk.len() == n * sb, "message and key encodings");  // len-guard
    assert!(rand.len() == n * (k + 1) * 48, "randomness encodings");  // len-guard
    let (mut cm, mut h, mut ct) = (vec![0u8; n * sb], vec![0u8; n * sb], vec![0u8; n * k * 2 * sb]);
    ctx.check(unsafe { cc_sigreq_new_batch(ctx.raw, n, q, k, m.as_ptr(), pk.as_ptr(), rand.as_ptr(),
                                           cm.as_mut_ptr(), h.as_mut_ptr(), ct.as_mut_ptr()) });
    let blind: Vec<u8> = (0..n * (3 * k + 2)).flat_map(|_| FieldElement::random().to_bytes()).collect();
    let mut proofs = vec![0u8; n * pb];
    assert!(blind.len() == n * (3 * k + 2) * 48, "blinding encodings");  // len-guard
    assert!(h.len() == n * sb && proofs.len() == n * pb, "h and proof records");  // len-guard
    ctx.check(unsafe { cc_sigreq_pok_init_batch(ctx.raw, n, q, k, h.as_ptr(), pk.as_ptr(), blind.as_ptr(),
                                                proofs.as_mut_ptr()) });
    // to_bytes: g | T_sk | h_0 .. h_{k-1} | g | T_comm | k x (g | T_1i | pk | h | T_2i)
    let chals: Vec<FieldElement> = (0..n).map(|i| {
        let p = &proofs[i * pb..(i + 1) * pb];
        let mut row = [&gb[..], &p[..sb], &hb[..k * sb], &gb[..], &p[sb + 48..2 * sb + 48]].concat();
        for j in 0..k {
            let o = 2 * sb + 48 * (k + 2) + j * (2 * sb + 144);
            row.extend_from_slice(&[&gb[..], &p[o..o + sb], &pk[i * sb..(i + 1) * sb], &h[i * sb..(i + 1) * sb],
                                    &p[o + sb + 48..o + 2 * sb + 48]].concat());
        }
        FieldElement::from_msg_hash(&row)
    }).collect();
    let sk: Vec<u8> = elgamal_sks.iter().flat_map(|s| s.to_bytes()).collect();
    let ch: Vec<u8> = chals.iter().flat_map(|c| c.to_bytes()).collect();
    assert!(sk.len() == n * 48 && ch.len() == n * 48, "key and challenge encodings");  // len-guard
    ctx.check(unsafe { cc_sigreq_pok_gen_proof_batch(ctx.raw, n, q, k, m.as_ptr(), rand.as_ptr(), blind.as_ptr(),
                                                     sk.as_ptr(), ch.as_ptr(), proofs.as_mut_ptr()) });
    let pt = |b: &[u8]| SignatureGroup::from_bytes(b).unwrap();
    chals.into_iter().enumerate().map(|(i, c)| {
        let req = SignatureRequest {
            known_messages: messages[i][k..].to_vec().into(),
            commitment: pt(&cm[i * sb..(i + 1) * sb]),
            ciphertexts: (0..k).map(|j| { let o = (i * k + j) * 2 * sb; (pt(&ct[o..o + sb]), pt(&ct[o + sb..o + 2 * sb])) })
                .collect() };
        let rs = (0..k + 1).map(|j| FieldElement::from_bytes(&rand[(i * (k + 1) + j) * 48..(i * (k + 1) + j + 1) * 48])
                                .unwrap()).collect();
        (req, rs, proofs[i * pb..(i + 1) * pb].to_vec(), c)
    }).collect()
}

/// One dealt keygen: (secret_x, secret_y, signers) as trusted_party_SSS_keygen returns them, and with
/// Pedersen generators the coefficient commitments ((q + 1) x threshold, polynomial-major) and every
/// signer's blinding shares (x_t | y_t[q], signer-major) of trusted_party_PVSS_keygen.
pub type DealtKeygen = (FieldElement, Vec<FieldElement>, Vec<Signer>, Option<(Vec<G1>, Vec<FieldElement>)>);

/// trusted_party_SSS_keygen (keygen.rs:53-71; `vss` None) or trusted_party_PVSS_keygen (74-122; `vss` the
/// Pedersen generators g, h) for m independent committees of `total` signers with threshold `threshold`:
/// fresh polynomials per keygen (FieldElement::random), every share, commitment and verkey on the GPU.
pub fn keygen_deal_batch(m: usize, threshold: usize, total: usize, params: &Params, vss: Option<(&G1, &G1)>,
                         ctx: &HipCtx) -> Vec<DealtKeygen> {
    if m == 0 { return Vec::new(); }
    let (q, t, ob) = (params.h.len(), threshold, ctx.oth_bytes());
    assert!(t > 0 && t <= total, "threshold of total signers");  // len-guard
    let gt = params.g_tilde.to_bytes();
    let gh = vss.map(|(g, h)| (g.to_bytes(), h.to_bytes()));
    assert_eq!(gt.len(), ob, "g_tilde encoding");  // len-guard
    assert!(gh.iter().all(|(g, h)| g.len() == 97 && h.len() == 97), "Pedersen generator encodings");  // len-guard
    let null = std::ptr::null::<u8>();
    ctx.check(unsafe { cc_set_keygen_params(ctx.raw, gt.as_ptr(), gh.as_ref().map_or(null, |p| p.0.as_ptr()),
                                            gh.as_ref().map_or(null, |p| p.1.as_ptr()), 0) });
    let nc = m * (q + 1) * t;
    let cf: Vec<u8> = (0..nc).flat_map(|_| FieldElement::random().to_bytes()).collect();
    let ct: Vec<u8> = if vss.is_some() { (0..nc).flat_map(|_| FieldElement::random().to_bytes()).collect() }
                      else { Vec::new() };
    assert!(cf.len() == nc * 48 && (vss.is_none() || ct.len() == nc * 48), "coefficient encodings");  // len-guard
    let ns = m * total;
    let (mut x, mut y, mut xk, mut yk) = (vec![0u8; ns * 48], vec![0u8; ns * q * 48], vec![0u8; ns * ob],
                                          vec![0u8; ns * q * ob]);
    let pn = if vss.is_some() { 1 } else { 0 };
    let (mut xt, mut yt, mut cm) = (vec![0u8; pn * ns * 48], vec![0u8; pn * ns * q * 48], vec![0u8; pn * nc * 97]);
    assert!(x.len() == ns * 48 && y.len() == ns * q * 48 && xk.len() == ns * ob && yk.len() == ns * q * ob,
            "share and verkey outputs");  // len-guard
    assert!(vss.is_none() || (xt.len() == ns * 48 && yt.len() == ns * q * 48 && cm.len() == nc * 97),
            "blinding share and commitment outputs");  // len-guard
    let nm = std::ptr::null_mut::<u8>();
    ctx.check(unsafe { cc_keygen_deal_batch(ctx.raw, m, q, t, total, cf.as_ptr(),
                                            if vss.is_some() { ct.as_ptr() } else { null }, x.as_mut_ptr(),
                                            y.as_mut_ptr(), if vss.is_some() { xt.as_mut_ptr() } else { nm },
                                            if vss.is_some() { yt.as_mut_ptr() } else { nm },
                                            if vss.is_some() { cm.as_mut_ptr() } else { nm }, xk.as_mut_ptr(),
                                            yk.as_mut_ptr()) });
    let fe = |b: &[u8], i: usize| FieldElement::from_bytes(&b[i * 48..(i + 1) * 48]).unwrap();
    let og = |b: &[u8], i: usize| OtherGroup::from_bytes(&b[i * ob..(i + 1) * ob]).unwrap();
    (0..m).map(|k| {
        let signers = (0..total).map(|i| { let s = k * total + i; Signer {
            id: i + 1,
            sigkey: Sigkey { x: fe(&x, s), y: (0..q).map(|j| fe(&y, s * q + j)).collect() },
            verkey: Verkey { X_tilde: og(&xk, s), Y_tilde: (0..q).map(|j| og(&yk, s * q + j)).collect() } } }).collect();
        let sec = |p: usize| fe(&cf, (k * (q + 1) + p) * t);
        let ped = vss.map(|_| (
            (0..(q + 1) * t).map(|i| G1::from_bytes(&cm[(k * (q + 1) * t + i) * 97..(k * (q + 1) * t + i + 1) * 97])
                                 .unwrap()).collect(),
            (0..total).flat_map(|i| { let s = k * total + i;
                let mut v = vec![fe(&xt, s)];
                v.extend((0..q).map(|j| fe(&yt, s * q + j)));
                v }).collect()));
        (sec(0), (1..=q).map(sec).collect(), signers, ped)
    }).collect()
}

/// A caller-owned buffer in HBM: its device address and its length in bytes.  The shim allocates no
/// device memory; whoever does (a HIP binding, a tensor library) vouches for the pair once, here.
#[derive(Clone, Copy)]
pub struct DeviceBytes { ptr: *mut u8, len: usize }

impl DeviceBytes {
    /// Safety: `ptr` addresses `len` bytes of memory of the context's device, which stay allocated until
    /// the stream the buffer is used on has run.
    pub unsafe fn new(ptr: *mut u8, len: usize) -> DeviceBytes { DeviceBytes { ptr, len } }
    pub fn len(&self) -> usize { self.len }
    pub fn as_ptr(&self) -> *mut u8 { self.ptr }
}

/// The issuer's step for n requests resident in HBM (signature.rs:324-433): SignatureRequestProof::verify
/// against the context's request params (cc_set_request_params with this `params`), then
/// BlindSignature::new with the h the verify computed, both queued on `stream` (null: the context's)
/// with no host round trip.  Buffers in the layouts of cc_sigreq_verify_batch / cc_blind_sign_batch;
/// verdicts n bytes, h, c1, c2 n SignatureGroup encodings each.  Every request is signed: the caller
/// reads the verdicts and drops the refused ones.
pub fn issuer_verify_sign_device(n: usize, k: usize, commitment: DeviceBytes, known: DeviceBytes,
                                 ciphertexts: DeviceBytes, elgamal_pk: DeviceBytes, proofs: DeviceBytes,
                                 chal: DeviceBytes, verdicts: DeviceBytes, h: DeviceBytes, c1: DeviceBytes,
                                 c2: DeviceBytes, sigkey: &Sigkey, params: &Params, ctx: &HipCtx,
                                 stream: *mut std::os::raw::c_void) {
    let q = params.h.len();
    let sb = ctx.sig_bytes();
    let gb = params.g.to_bytes();
    let hb: Vec<u8> = params.h.iter().flat_map(|p| p.to_bytes()).collect();
    assert!(q > 0 && k <= q, "k hidden of q messages");  // len-guard
    assert_eq!(sigkey.y.len(), q, "Sigkey valid for {} messages", q);  // len-guard
    assert!(gb.len() == sb && hb.len() == q * sb, "params encodings");  // len-guard
    ctx.check(unsafe { cc_set_request_params(ctx.raw, q, gb.as_ptr(), hb.as_ptr(), 0) });
    let pb = unsafe { cc_sigreq_proof_bytes(ctx.raw, k) };
    assert!(commitment.len() >= n * sb && known.len() >= n * (q - k) * 48, "commitments and known messages");  // len-guard
    assert!(ciphertexts.len() >= n * k * 2 * sb && elgamal_pk.len() >= n * sb, "ciphertexts and ElGamal keys");  // len-guard
    assert!(proofs.len() >= n * pb && chal.len() >= n * 48, "proof records and challenges");  // len-guard
    assert!(verdicts.len() >= n && h.len() >= n * sb, "verdicts and h");  // len-guard
    assert!(c1.len() >= n * sb && c2.len() >= n * sb, "blind signature halves");  // len-guard
    ctx.check(unsafe { cc_sigreq_verify_batch_device(ctx.raw, n, q, k, commitment.as_ptr(), known.as_ptr(),
                                                     ciphertexts.as_ptr(), elgamal_pk.as_ptr(), proofs.as_ptr(),
                                                     chal.as_ptr(), verdicts.as_ptr(), h.as_ptr(), stream) });
    let x = sigkey.x.to_bytes();
    let y: Vec<u8> = sigkey.y.iter().flat_map(|v| v.to_bytes()).collect();
    assert!(x.len() == 48 && y.len() == q * 48, "signing key encodings");  // len-guard
    ctx.check(unsafe { cc_blind_sign_batch_device(ctx.raw, n, q, k, commitment.as_ptr(), known.as_ptr(),
                                                  ciphertexts.as_ptr(), h.as_ptr(), x.as_ptr(), y.as_ptr(),
                                                  h.as_ptr(), c1.as_ptr(), c2.as_ptr(), stream) });
}

#[allow(dead_code)]
const _MODE_TYPE: c_int = CC_SIG_G2;
