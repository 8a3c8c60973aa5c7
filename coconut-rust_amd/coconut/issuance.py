"""Issuance batch entry points — host mirror of reference src/signature.rs:124-444 (SURVEY.md
§8(f) row 3).  Issuer side: BlindSignature::new (382-433) and SignatureRequestProof::verify (324-377)
for whole batches of signature requests.  Holder side: SignatureRequest::new (124-192),
SignatureRequestPoK::init / to_bytes / gen_proof (216-320) and BlindSignature::unblind (436-443).  All
through include/coconut_hip.h."""
from __future__ import annotations

import ctypes
import secrets
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np

from ._lib import buf, check, lib, need
from .errors import CoconutError
from .signature import R_ORDER, Context, Params, fr_bytes, hash_msg


def blind_sign_batch(ctx: Context, q: int, k: int, commitments: Sequence[bytes], known: Sequence[Sequence[bytes]],
                     ciphertexts: Sequence[Sequence[tuple]], x: bytes, y: Sequence[bytes]):
    """Per request: (h, c~1, c~2) = BlindSignature::new(request, Sigkey{x, y}); returns three lists."""
    n = len(commitments)
    sb = ctx.mode.sig_bytes
    cm = b"".join(commitments)
    kn = b"".join(m for row in known for m in row)
    ct = b"".join(a + b for row in ciphertexts for a, b in row)
    yb = b"".join(y)
    for v, nb, what in ((cm, n * sb, "commitments"), (kn, n * max(q - k, 0) * 48, "known messages"),
                        (ct, n * k * 2 * sb, "ciphertexts"), (x, 48, "x"), (yb, q * 48, "y")):
        need(v, nb, what)
    outs = [np.zeros(max(n, 1) * sb, dtype=np.uint8) for _ in range(3)]
    keep = [buf(v) for v in (cm, kn, ct, x, yb)]
    check(lib.cc_blind_sign_batch(ctx.h, n, q, k, keep[0][0], keep[1][0] if kn else None, keep[2][0] if ct else None,
                                  keep[3][0], keep[4][0], *[ctypes.c_void_p(o.ctypes.data) for o in outs]),
          "cc_blind_sign_batch")
    raw = [o.tobytes() for o in outs]
    return tuple([r[i * sb:(i + 1) * sb] for i in range(n)] for r in raw)


def sigreq_verify_batch(ctx: Context, q: int, k: int, g: bytes, h: Sequence[bytes], commitments: Sequence[bytes],
                        known: Sequence[Sequence[bytes]], ciphertexts: Sequence[Sequence[tuple]],
                        elgamal_pks: Sequence[bytes], proofs: Sequence[bytes], chals: Sequence[bytes]) -> np.ndarray:
    """SignatureRequestProof::verify per request; proofs packed as cc_sigreq_proof_bytes describes."""
    n = len(commitments)
    pb = lib.cc_sigreq_proof_bytes(ctx.h, k)
    if any(len(p) != pb for p in proofs):
        raise ValueError(f"each proof must be {pb} bytes")
    kn = b"".join(m for row in known for m in row)
    ct = b"".join(a + b for row in ciphertexts for a, b in row)
    sb = ctx.mode.sig_bytes
    parts = (g, b"".join(h[:k]), b"".join(commitments), kn, ct, b"".join(elgamal_pks), b"".join(proofs),
             b"".join(chals))
    for v, nb, what in zip(parts, (sb, k * sb, n * sb, n * max(q - k, 0) * 48, n * k * 2 * sb, n * sb, n * pb,
                                   n * 48),
                           ("g", "h", "commitments", "known messages", "ciphertexts", "ElGamal keys", "proofs",
                            "challenges")):
        need(v, nb, what)
    keep = [buf(v) for v in parts]
    v = np.zeros(max(n, 1), dtype=np.uint8)
    ptr = [kp[0] for kp in keep]
    check(lib.cc_sigreq_verify_batch(ctx.h, n, q, k, ptr[0], ptr[1] if k else None, ptr[2], ptr[3] if kn else None,
                                     ptr[4] if ct else None, ptr[5], ptr[6], ptr[7], ctypes.c_void_p(v.ctypes.data)),
          "cc_sigreq_verify_batch")
    return v[:n]


def _dev_need(checks):
    """need() for device tensors, [(tensor or None, bytes the call reads, name)]: each torch.uint8 and
    contiguous, every length first, then every tensor the call reads on a GPU."""
    for t, nbytes, what in checks:
        if t is None:
            need(None, nbytes, what)
        elif str(t.dtype) != "torch.uint8" or not t.is_contiguous():
            raise CoconutError(-4, f"{what}: a contiguous torch.uint8 tensor is required")
        elif nbytes > 0 and t.numel() < nbytes:
            raise CoconutError(-4, f"{what}: {t.numel()} bytes, the call reads {nbytes}")
    for t, nbytes, what in checks:
        if t is not None and nbytes > 0 and not t.is_cuda:
            raise CoconutError(-4, f"{what}: a device tensor is required")


def _dev_ptr(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _stream_ptr(stream):
    return None if stream is None else ctypes.c_void_p(stream.cuda_stream)


def sigreq_verify_batch_device(ctx: Context, n: int, q: int, k: int, commitments, known, ciphertexts, elgamal_pks,
                               proofs, chals, want_h: bool = False, stream=None):
    """SignatureRequestProof::verify for n requests whose inputs are torch.uint8 CUDA tensors in the layouts
    of sigreq_verify_batch (cc_sigreq_verify_batch_device), against the context's request params
    (Context.set_request_params): g and h_0 .. h_{k-1} come from there.  Asynchronous on `stream` (a
    torch.cuda.Stream; None: the context's).  Returns the verdict tensor (n bytes), or (verdicts, h) with
    want_h: h = compute_h(commitment, known) of every request, what blind_sign_batch_device takes."""
    import torch
    sb = ctx.mode.sig_bytes
    pb = sigreq_proof_bytes(ctx, k)
    _dev_need(((commitments, n * sb, "commitments"), (known, n * max(q - k, 0) * 48, "known messages"),
               (ciphertexts, n * k * 2 * sb, "ciphertexts"), (elgamal_pks, n * sb, "ElGamal keys"),
               (proofs, n * pb, "proofs"), (chals, n * 48, "challenges")))
    dev = commitments.device if n else None
    v = torch.empty(n, dtype=torch.uint8, device=dev)  # no fill kernel: it would run on another stream
    h = torch.empty(n * sb, dtype=torch.uint8, device=dev) if want_h else None
    check(lib.cc_sigreq_verify_batch_device(ctx.h, n, q, k, _dev_ptr(commitments), _dev_ptr(known),
                                            _dev_ptr(ciphertexts), _dev_ptr(elgamal_pks), _dev_ptr(proofs),
                                            _dev_ptr(chals), _dev_ptr(v), _dev_ptr(h), _stream_ptr(stream)),
          "cc_sigreq_verify_batch_device")
    return (v, h) if want_h else v


def blind_sign_batch_device(ctx: Context, n: int, q: int, k: int, commitments, known, ciphertexts, x: bytes,
                            y: Sequence[bytes], h=None, stream=None):
    """BlindSignature::new for n requests in HBM (cc_blind_sign_batch_device): torch.uint8 CUDA tensors in the
    layouts of blind_sign_batch, the issuer's key x, y as host bytes.  h: the tensor sigreq_verify_batch_device
    returned with want_h (None: h is hashed here; commitments may be None when h is given).  Asynchronous on
    `stream`.  Returns the tensors (h, c~1, c~2), n encodings each."""
    import torch
    sb = ctx.mode.sig_bytes
    yb = b"".join(y)
    need(x, 48, "x")
    need(yb, q * 48, "y")
    _dev_need(((commitments, 0 if h is not None else n * sb, "commitments"),
               (known, n * max(q - k, 0) * 48, "known messages"), (ciphertexts, n * k * 2 * sb, "ciphertexts"),
               (h, n * sb if h is not None else 0, "h")))
    src = h if h is not None else commitments
    dev = src.device if n else None
    outs = [torch.empty(n * sb, dtype=torch.uint8, device=dev) for _ in range(3)]
    keep = [buf(bytes(x)), buf(yb)]
    check(lib.cc_blind_sign_batch_device(ctx.h, n, q, k, _dev_ptr(commitments), _dev_ptr(known), _dev_ptr(ciphertexts),
                                         _dev_ptr(h), keep[0][0], keep[1][0], *[_dev_ptr(o) for o in outs],
                                         _stream_ptr(stream)), "cc_blind_sign_batch_device")
    return tuple(outs)


def vss_verify_batch(ctx: Context, t: int, g: bytes, h: bytes, commitment_sets: Sequence[Sequence[bytes]],
                     set_of: Sequence[int], ids: Sequence[int], shares: Sequence[tuple]) -> np.ndarray:
    """PedersenVSS::verify_share for a batch of (id, (s, s')) against their dealer's commitments (G1)."""
    n = len(ids)
    cm = b"".join(c for cs in commitment_sets for c in cs)
    so = np.ascontiguousarray(np.asarray(set_of, dtype=np.uint32))
    iv = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
    sh = b"".join(a + b for a, b in shares)
    for v, nb, what in ((g, 97, "g"), (h, 97, "h"), (cm, len(commitment_sets) * t * 97, "commitments"),
                        (sh, n * 96, "shares")):
        need(v, nb, what)
    if len(so) < n:
        need(None, n, "set_of")
    keep = [buf(v) for v in (g, h, cm, sh)]
    v = np.zeros(max(n, 1), dtype=np.uint8)
    check(lib.cc_vss_verify_batch(ctx.h, n, t, keep[0][0], keep[1][0], keep[2][0], len(commitment_sets),
                                  ctypes.c_void_p(so.ctypes.data), ctypes.c_void_p(iv.ctypes.data), keep[3][0],
                                  ctypes.c_void_p(v.ctypes.data)), "cc_vss_verify_batch")
    return v[:n]


def _set_begin(set_begin, n_sets: int, n: int) -> np.ndarray:
    """The CSR offsets as the C ABI reads them: n_sets + 1 uint64 on the host."""
    sb = np.ascontiguousarray(np.asarray(set_begin, dtype=np.uint64))
    if len(sb) != n_sets + 1:
        raise CoconutError(-4, f"set_begin: {len(sb)} entries for {n_sets} sets ({n} rows)")
    return sb


def vss_verify_sets(ctx: Context, t: int, commitment_sets: Sequence[Sequence[bytes]], set_begin: Sequence[int],
                    ids: Sequence[int], shares: Sequence[tuple], rlc: bool = False, want_stats: bool = False):
    """PedersenVSS::verify_share for the shares of whole commitment sets, under the g, h bound by
    Context.set_keygen_params (cc_vss_verify_sets): rows [set_begin[j], set_begin[j + 1]) belong to
    commitment_sets[j].  rlc: one random-linear-combination check a set first, per share only where it fails.
    Returns the verdicts, or (verdicts, stats) with want_stats: stats = (sets, sets the RLC check rejected,
    irregular sets, shares verified per share)."""
    n, ns = len(ids), len(commitment_sets)
    cm = b"".join(c for cs in commitment_sets for c in cs)
    sb = _set_begin(set_begin, ns, n)
    iv = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
    sh = b"".join(a + b for a, b in shares)
    need(cm, ns * t * 97, "commitments")
    need(sh, n * 96, "shares")
    keep = [buf(cm), buf(sh)]
    v = np.zeros(max(n, 1), dtype=np.uint8)
    st = np.zeros(4, dtype=np.uint32)
    check(lib.cc_vss_verify_sets(ctx.h, n, t, ns, ctypes.c_void_p(sb.ctypes.data), keep[0][0],
                                 ctypes.c_void_p(iv.ctypes.data), keep[1][0], 1 if rlc else 0,
                                 ctypes.c_void_p(v.ctypes.data), ctypes.c_void_p(st.ctypes.data)),
          "cc_vss_verify_sets")
    return (v[:n], tuple(int(x) for x in st)) if want_stats else v[:n]


def vss_verify_sets_device(ctx: Context, n: int, t: int, n_sets: int, set_begin: Sequence[int], commitments, ids,
                           shares, rlc: bool = False, seed: Optional[bytes] = None, stream=None):
    """vss_verify_sets on CUDA tensors (cc_vss_verify_sets_device): commitments n_sets x t x 97 and shares
    n x (s | s') as torch.uint8, ids as a torch.int64 / uint64 tensor of n entries; set_begin stays on the host.
    seed: 32 bytes keying the deltas (None with rlc: drawn here).  The call synchronises `stream` once.
    Returns (verdict tensor, stats)."""
    import torch
    sb = _set_begin(set_begin, n_sets, n)
    _dev_need(((commitments, n_sets * t * 97 if n else 0, "commitments"), (shares, n * 96, "shares")))
    if n and (ids is None or ids.element_size() != 8 or ids.numel() < n or not ids.is_contiguous() or not ids.is_cuda):
        raise CoconutError(-4, "ids: a contiguous device tensor of n 64-bit entries is required")
    if rlc and seed is None:
        seed = secrets.token_bytes(32)
    if seed is not None:
        need(seed, 32, "seed")
    keep = buf(bytes(seed)) if seed is not None else (None, None)
    v = torch.empty(n, dtype=torch.uint8, device=shares.device if n else None)
    st = np.zeros(4, dtype=np.uint32)
    check(lib.cc_vss_verify_sets_device(ctx.h, n, t, n_sets, ctypes.c_void_p(sb.ctypes.data), _dev_ptr(commitments),
                                        _dev_ptr(ids), _dev_ptr(shares), 1 if rlc else 0, keep[0], _dev_ptr(v),
                                        ctypes.c_void_p(st.ctypes.data), _stream_ptr(stream)),
          "cc_vss_verify_sets_device")
    return v, tuple(int(x) for x in st)


def unblind_batch(ctx: Context, c1s: Sequence[bytes], c2s: Sequence[bytes], sks: Sequence[bytes]) -> List[bytes]:
    """BlindSignature::unblind per row: sigma_2 = c~2 - sk * c~1 with that row's ElGamal secret key
    (48 B big-endian); sigma_1 is the blind signature's h."""
    n = len(c1s)
    sb = ctx.mode.sig_bytes
    if len(c2s) != n or len(sks) != n:
        raise ValueError("c1s, c2s and sks must have one entry per blind signature")
    a, b, k = b"".join(c1s), b"".join(c2s), b"".join(sks)
    for v, nb, what in ((a, n * sb, "c1"), (b, n * sb, "c2"), (k, n * 48, "ElGamal secret keys")):
        need(v, nb, what)
    out = np.zeros(max(n, 1) * sb, dtype=np.uint8)
    keep = [buf(v) for v in (a, b, k)]
    check(lib.cc_unblind_batch(ctx.h, n, keep[0][0], keep[1][0], keep[2][0], ctypes.c_void_p(out.ctypes.data)),
          "cc_unblind_batch")
    raw = out.tobytes()
    return [raw[i * sb:(i + 1) * sb] for i in range(n)]


# ---------------------------------------------------------------- holder side: the signature request
def _fresh_scalars(count: int) -> bytes:
    """count scalars from the OS generator: 48 random bytes each, reduced mod r (bias < 2^-128)."""
    return b"".join((int.from_bytes(secrets.token_bytes(48), "big") % R_ORDER).to_bytes(48, "big")
                    for _ in range(count))


def sigreq_proof_bytes(ctx: Context, k: int) -> int:
    """Bytes of one request's proof record, 2 sb + 48 (k + 2) + k (2 sb + 144) (cc_sigreq_proof_bytes)."""
    sb = ctx.mode.sig_bytes
    return 2 * sb + 48 * (k + 2) + k * (2 * sb + 144)


def sigreq_new_batch(ctx: Context, n: int, q: int, k: int, msgs: bytes, elgamal_pk: bytes,
                     rand: Optional[bytes] = None):
    """SignatureRequest::new for n requests with the first k of q messages hidden, under the context's
    request params (Context.set_request_params; cc_sigreq_new_batch).  msgs n x q x 48, elgamal_pk n
    encodings, rand n x (k + 1) x 48 = r | k_0 .. per request (None draws it from `secrets`).
    Returns (commitments, hs, ciphertexts, rand): n encodings, n encodings, n x k x (c1 | c2), and the
    randomness gen_proof needs."""
    sb = ctx.mode.sig_bytes
    if rand is None:
        rand = _fresh_scalars(n * (k + 1))
    for v, nb, what in ((msgs, n * q * 48, "messages"), (elgamal_pk, n * sb if k else 0, "ElGamal keys"),
                        (rand, n * (k + 1) * 48, "randomness")):
        need(v, nb, what)
    outs = [np.zeros(max(n * w, 1), dtype=np.uint8) for w in (sb, sb, k * 2 * sb)]
    keep = [buf(x) for x in (msgs, elgamal_pk, rand)]
    check(lib.cc_sigreq_new_batch(ctx.h, n, q, k, keep[0][0], keep[1][0], keep[2][0],
                                  *[ctypes.c_void_p(o.ctypes.data) for o in outs]), "cc_sigreq_new_batch")
    cm, h, ct = (o.tobytes()[:n * w] for o, w in zip(outs, (sb, sb, k * 2 * sb)))
    return cm, h, ct, bytes(rand)


def sigreq_pok_init_batch(ctx: Context, n: int, q: int, k: int, h: bytes, elgamal_pk: bytes,
                          blind: Optional[bytes] = None):
    """SignatureRequestPoK::init for n requests (cc_sigreq_pok_init_batch): h = the hs of sigreq_new_batch,
    blind n x (3k + 2) x 48 = b_sk | hb_0 .. hb_{k-1} | b_r | k x (b1_i | b2_i) (None draws it).
    Returns (proofs, blind): n proof records with the T fields filled and the responses zero."""
    sb = ctx.mode.sig_bytes
    if blind is None:
        blind = _fresh_scalars(n * (3 * k + 2))
    for v, nb, what in ((h, n * sb if k else 0, "h"), (elgamal_pk, n * sb if k else 0, "ElGamal keys"),
                        (blind, n * (3 * k + 2) * 48, "blindings")):
        need(v, nb, what)
    pb = sigreq_proof_bytes(ctx, k)
    out = np.zeros(max(n * pb, 1), dtype=np.uint8)
    keep = [buf(x) for x in (h, elgamal_pk, blind)]
    check(lib.cc_sigreq_pok_init_batch(ctx.h, n, q, k, keep[0][0], keep[1][0], keep[2][0],
                                       ctypes.c_void_p(out.ctypes.data)), "cc_sigreq_pok_init_batch")
    return out.tobytes()[:n * pb], bytes(blind)


def sigreq_pok_gen_proof_batch(ctx: Context, n: int, q: int, k: int, msgs: bytes, rand: bytes, blind: bytes,
                               elgamal_sk: bytes, chal: bytes, proofs: bytes) -> bytes:
    """SignatureRequestPoK::gen_proof for n committed proofs (cc_sigreq_pok_gen_proof_batch): fills the
    response fields of `proofs` (b - chal * secret mod r) and returns the records, which
    sigreq_verify_batch accepts as they are."""
    pb = sigreq_proof_bytes(ctx, k)
    for v, nb, what in ((msgs, n * q * 48, "messages"), (rand, n * (k + 1) * 48, "randomness"),
                        (blind, n * (3 * k + 2) * 48, "blindings"), (elgamal_sk, n * 48, "ElGamal secret keys"),
                        (chal, n * 48, "challenges"), (proofs, n * pb, "proofs")):
        need(v, nb, what)
    out = np.frombuffer(bytes(proofs[:n * pb]) or bytes(1), dtype=np.uint8).copy()
    keep = [buf(x) for x in (msgs, rand, blind, elgamal_sk, chal)]
    check(lib.cc_sigreq_pok_gen_proof_batch(ctx.h, n, q, k, keep[0][0], keep[1][0], keep[2][0], keep[3][0],
                                            keep[4][0], ctypes.c_void_p(out.ctypes.data)),
          "cc_sigreq_pok_gen_proof_batch")
    return out.tobytes()[:n * pb]


def sigreq_pok_to_bytes_batch(ctx: Context, n: int, k: int, g: bytes, h_params: Sequence[bytes], hs: bytes,
                              elgamal_pk: bytes, proofs: bytes) -> List[bytes]:
    """SignatureRequestPoK::to_bytes per request: every committed part is its bases in commit order, then
    its T: g | T_sk | h_0 .. h_{k-1} | g | T_comm | k x (g | T_1i | pk | h | T_2i)."""
    sb = ctx.mode.sig_bytes
    pb = sigreq_proof_bytes(ctx, k)
    hp = b"".join(bytes(x) for x in h_params[:k])
    for v, nb, what in ((g, sb, "g"), (hp, k * sb, "h"), (hs, n * sb, "h"), (elgamal_pk, n * sb, "ElGamal keys"),
                        (proofs, n * pb, "proofs")):
        need(v, nb, what)
    g = bytes(g)
    rows = []
    for i in range(n):
        p = proofs[i * pb:(i + 1) * pb]
        pk, h = elgamal_pk[i * sb:(i + 1) * sb], hs[i * sb:(i + 1) * sb]
        row = [g, p[:sb], hp, g, p[sb + 48:2 * sb + 48]]
        for j in range(k):
            o = 2 * sb + 48 * (k + 2) + j * (2 * sb + 144)
            row += [g, p[o:o + sb], pk, h, p[o + sb + 48:o + 2 * sb + 48]]
        rows.append(b"".join(bytes(x) for x in row))
    return rows


def sigreq_challenge_batch(ctx: Context, n: int, k: int, g: bytes, h_params: Sequence[bytes], hs: bytes,
                           elgamal_pk: bytes, proofs: bytes) -> bytes:
    """The reference's challenge (signature.rs:617: FieldElement::from_msg_hash(&pok.to_bytes())) for n
    committed proofs: the to_bytes rows through hash_msg on the GPU; n x 48 B."""
    return b"".join(hash_msg(ctx, sigreq_pok_to_bytes_batch(ctx, n, k, g, h_params, hs, elgamal_pk, proofs)))


@dataclass
class SignatureRequest:
    """signature.rs:107-112: what the holder sends the signers."""
    known_messages: List[bytes]
    commitment: bytes
    ciphertexts: List[tuple]  # (c1, c2) per hidden message
    h: bytes                  # compute_h(commitment, known), what the signers recompute

    @staticmethod
    def new(msgs: Sequence[Union[int, bytes]], count_hidden: int, elgamal_pk: bytes, params: Params,
            ctx: Context = None, rand: Optional[Sequence[Union[int, bytes]]] = None):
        """Returns (request, randomness) as the reference does; randomness = [r, k_0 ..] as 48-byte
        scalars.  rand fixes the draws (replaying a recorded request)."""
        ctx = ctx or Context.default()
        q, k = len(msgs), int(count_hidden)
        if q != len(params.h) or k > q:
            raise CoconutError(-1, f"{q} messages, {k} hidden, params for {len(params.h)}")
        if rand is not None and len(rand) != k + 1:
            raise CoconutError(-2, f"rand holds {len(rand)} scalars, new draws {k + 1}")
        ctx.set_request_params(params.g, params.h)
        mb = b"".join(fr_bytes(m) for m in msgs)
        rb = None if rand is None else b"".join(fr_bytes(x) for x in rand)
        cm, h, ct, rb = sigreq_new_batch(ctx, 1, q, k, mb, elgamal_pk, rb)
        sb = ctx.mode.sig_bytes
        cts = [(ct[2 * i * sb:(2 * i + 1) * sb], ct[(2 * i + 1) * sb:(2 * i + 2) * sb]) for i in range(k)]
        req = SignatureRequest([mb[i * 48:(i + 1) * 48] for i in range(k, q)], cm, cts, h)
        return req, [rb[i * 48:(i + 1) * 48] for i in range(k + 1)]


@dataclass
class SignatureRequestPoK:
    """signature.rs:205-213: the committed state between init and gen_proof."""
    proof: bytes             # the proof record: T fields set, responses zero until gen_proof
    k: int
    q: int
    g: bytes
    h_params: List[bytes]
    h: bytes
    elgamal_pk: bytes
    blind: bytes             # b_sk | hb_0 .. | b_r | k x (b1_i | b2_i) (secret)
    ctx: Context = None

    @staticmethod
    def init(sig_req: SignatureRequest, elgamal_pk: bytes, params: Params, ctx: Context = None,
             blind: Optional[Sequence[Union[int, bytes]]] = None) -> "SignatureRequestPoK":
        ctx = ctx or Context.default()
        k = len(sig_req.ciphertexts)
        q = k + len(sig_req.known_messages)
        if blind is not None and len(blind) != 3 * k + 2:
            raise CoconutError(-2, f"blind holds {len(blind)} scalars, init draws {3 * k + 2}")
        ctx.set_request_params(params.g, params.h)
        bb = None if blind is None else b"".join(fr_bytes(x) for x in blind)
        proof, bb = sigreq_pok_init_batch(ctx, 1, q, k, sig_req.h, elgamal_pk, bb)
        return SignatureRequestPoK(proof, k, q, bytes(params.g), [bytes(x) for x in params.h], sig_req.h,
                                   bytes(elgamal_pk), bb, ctx)

    def to_bytes(self) -> bytes:
        ctx = self.ctx or Context.default()
        return sigreq_pok_to_bytes_batch(ctx, 1, self.k, self.g, self.h_params, self.h, self.elgamal_pk, self.proof)[0]

    def gen_proof(self, hidden_msgs: Sequence[Union[int, bytes]], randomness: Sequence[Union[int, bytes]],
                  elgamal_sk: Union[int, bytes], chal: Union[int, bytes]) -> bytes:
        """hidden_msgs: the k hidden messages; randomness: what SignatureRequest.new returned.  Returns the
        proof record sigreq_verify_batch reads."""
        ctx = self.ctx or Context.default()
        if len(hidden_msgs) != self.k or len(randomness) != self.k + 1:
            raise CoconutError(-2, f"{len(hidden_msgs)} hidden messages and {len(randomness)} scalars for k = {self.k}")
        # gen_proof reads the first k of q messages; the known ones are not part of any response
        mb = b"".join(fr_bytes(m) for m in hidden_msgs) + bytes(48 * (self.q - self.k))
        rb = b"".join(fr_bytes(x) for x in randomness)
        return sigreq_pok_gen_proof_batch(ctx, 1, self.q, self.k, mb, rb, self.blind, fr_bytes(elgamal_sk),
                                          fr_bytes(chal), self.proof)
