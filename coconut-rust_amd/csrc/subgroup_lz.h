// Order-r subgroup membership of a G1 point on the lazy field (subgroup.h's test over curve_lz.h) — device
// code shared by the PoK RLC prep (pok_rlc.hip: J) and the Pedersen VSS commitment prep (vss.hip).
#pragma once
#include "curve_lz.h"
#include "pairing.h"  // X_ABS

namespace cc {

// a storage-form affine G1 point on the lazy field (a canonical operand of lz::jg_add_aff)
DEV lz::AG ag_from_aff(const Aff<Fp>& a) {
    return {lz::fit<lz::AN, lz::BC>(lz::reduce(lz::in_r(a.x))), lz::fit<lz::AN, lz::BC>(lz::reduce(lz::in_r(a.y)))};
}

// [|x|] A on the lazy field (subgroup.h jac_mul_xabs): 63 doublings, 5 additions
DEV lz::JG jg_mul_xabs(const lz::JG& a) {
    lz::JG acc = a;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        acc = lz::jg_dbl(acc);
        if ((X_ABS >> b) & 1ull) acc = lz::jg_add(acc, a);
    }
    return acc;
}

// subgroup.h g1_in_subgroup on the lazy field: phi(P) == -[x^2] P, phi(x, y) = (beta x, y)
DEV bool g1_in_subgroup_lz(const Aff<Fp>& p) {
    constexpr uint32_t BETA[NL] = {0x6abf79e7u, 0x9b29629du, 0xaef3ac5au, 0x568c22e6u, 0x4212c814u, 0x9bb87339u,
                                   0x891f2cfbu, 0xfbdce22eu, 0x21d96a8du, 0x364cdfb4u, 0xbed57a58u, 0x1946806fu};
    lz::JG t = lz::jg_add_aff(lz::jg_inf(), ag_from_aff(p));
    t = jg_mul_xabs(jg_mul_xabs(t));  // [x^2] P
    Aff<Fp> ph;
    Fp beta;
#pragma unroll
    for (int j = 0; j < NL; j++) beta.v[j] = BETA[j];
    fp_mul(ph.x, p.x, beta);
    ph.y = p.y;
    t = lz::jg_add_aff(t, ag_from_aff(ph));  // [x^2] P + phi(P) == O
    return lz::jg_is_inf(t);
}

}  // namespace cc
