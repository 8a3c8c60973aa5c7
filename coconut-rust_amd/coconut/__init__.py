"""coconut (MI355X) — host-side mirror of the reference crate's verifier API over the HIP C ABI.

Mirrors 3for/coconut-rust (`/root/reference/src/lib.rs:26-31` module list) for the hot path only:
`signature` (Signature::verify / aggregate, Verkey::aggregate + batch entry points), `pok_sig`
(PoKOfSignature::init / gen_proof, PoKOfSignatureProof::verify), `issuance` (issuer-side batches, the
holder's SignatureRequest::new, SignatureRequestPoK and BlindSignature::unblind), `keygen`
(trusted_party_SSS_keygen / trusted_party_PVSS_keygen and the decentralized keygen's combine), `errors`.  Every computation runs in libcoconut_hip.so on the GPU; importing
this package on a machine without the built library raises immediately.
"""
from .errors import CoconutError, CoconutErrorKind  # noqa: F401
from ._lib import version, source_hash  # noqa: F401
from .signature import (GroupMode, Params, Verkey, Signature, Context, verify_batch, verify_batch_locate,  # noqa: F401
                        signature_aggregate_batch, verkey_aggregate_batch, verkey_aggregate_ids, fixed_base_mul, subgroup_check, hash_to_curve, hash_msg, params_new,
                        G1_GENERATOR, G2_GENERATOR)
from .pok_sig import (PoKOfSignature, PoKOfSignatureProof, pok_verify_batch, pok_verify_batch_locate,  # noqa: F401
                      pok_init_batch,
                      pok_gen_proof_batch, pok_challenge_batch, pok_to_bytes_batch)
from .dist import DeviceEngine, PokDeviceEngine  # noqa: F401
from .issuance import (blind_sign_batch, sigreq_verify_batch, vss_verify_batch, unblind_batch,  # noqa: F401
                       SignatureRequest, SignatureRequestPoK, sigreq_new_batch, sigreq_pok_init_batch,
                       sigreq_pok_gen_proof_batch, sigreq_pok_to_bytes_batch, sigreq_challenge_batch,
                       sigreq_proof_bytes, sigreq_verify_batch_device, blind_sign_batch_device,
                       vss_verify_sets, vss_verify_sets_device)
from .keygen import (Signer, Sigkey, keygen_deal_batch, keygen_combine_batch,  # noqa: F401
                     keygen_deal_batch_device, keygen_combine_batch_device, keygen_verify_shares_device,
                     trusted_party_SSS_keygen, trusted_party_PVSS_keygen)
