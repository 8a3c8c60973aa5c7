// Byte offsets inside one request's SignatureRequestProof record (the layout cc_sigreq_verify_batch
// reads and cc_sigreq_pok_init_batch / cc_sigreq_pok_gen_proof_batch write):
//   T_sk | r_sk | T_comm | r_comm[0..k] | k x (T_1 | r_1 | T_2 | r_2a | r_2b)
#pragma once
#include <cstddef>

namespace cc {

struct ProofLayout {
    size_t sb, k;
    __host__ __device__ size_t t_sk() const { return 0; }
    __host__ __device__ size_t r_sk() const { return sb; }
    __host__ __device__ size_t t_comm() const { return sb + 48; }
    __host__ __device__ size_t r_comm(size_t i) const { return 2 * sb + 48 + 48 * i; }
    __host__ __device__ size_t ct(size_t i) const { return 2 * sb + 48 * (k + 2) + i * (2 * sb + 144); }
    __host__ __device__ size_t bytes() const { return ct(k); }
};

}  // namespace cc
