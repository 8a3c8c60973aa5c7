// Device self-test of the lazy radix-2^28 field core (lazy.h) and of the divstep inversions (field.h
// fp_inv_int, tower_q.h fp_inv_int_quad) — test infrastructure exported through the C ABI
// (cc_selftest_lazy) so tests/test_gpu_lazy.py can drive the kernels' exact code on the device with
// inputs at the limits the compile-time bounds allow and check them against Python big integers.
// Not on any verification path.  cc_selftest_field (below) does the same for the canonical Fp of
// field.h and the scalar field of fr.h / codec.h (tests/test_gpu_field_edges.py).
#include "fr.h"
#include "tower_q.h"

namespace {

// op 0: (a b + c d) / R' (lz_mont<2>); op 1: a b / R' (lz_mont<1>); op 2: reduce(a); op 3: squeeze(a);
// op 4: fp_inv_int(a) and op 5: fp_inv_int_quad(a) on a plain integer a < p in limbs 0..11 (op 5: the
// four lanes of each quad must hold the same a); op 6: canon(a), the residue in [0, p) as 12 words in
// limbs 0..11.
// One kernel per op: with a runtime op the four paths shared one exit block and hipcc (ROCm 7.2)
// left limb 0 of the squeeze path in an undefined register (an implicit-def merged at the shared
// store) — separate instantiations keep each path's control flow trivial.
template <int op>
__global__ __launch_bounds__(256) void k_lz_selftest(size_t n, const int32_t* __restrict__ a,
                                                     const int32_t* __restrict__ b, const int32_t* __restrict__ c,
                                                     const int32_t* __restrict__ d, int32_t* __restrict__ out) {
    using namespace cc::lz;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t x[LN], y[LN], u[LN], v[LN];
#pragma unroll
    for (int k = 0; k < LN; k++) {
        x[k] = a[i * LN + k];
        y[k] = b[i * LN + k];
        u[k] = c[i * LN + k];
        v[k] = d[i * LN + k];
    }
    W14 r;
    if constexpr (op == 4 || op == 5) {
        cc::Fp fa, fr;
#pragma unroll
        for (int k = 0; k < cc::NL; k++) fa.v[k] = (uint32_t)x[k];
        if constexpr (op == 4) cc::fp_inv_int(fr, fa);
        else fp_inv_int_quad(fr, fa);
#pragma unroll
        for (int k = 0; k < LN; k++) r.v[k] = k < cc::NL ? (int32_t)fr.v[k] : 0;
    } else if constexpr (op == 6) {
        Fq<2047, 32768> q;
#pragma unroll
        for (int k = 0; k < LN; k++) q.v[k] = x[k];
        const cc::Fp fr = canon(q);
#pragma unroll
        for (int k = 0; k < LN; k++) r.v[k] = k < cc::NL ? (int32_t)fr.v[k] : 0;
    } else if constexpr (op == 0) {
        r = lz_mont<2>(x, y, u, v);
    } else if constexpr (op == 1) {
        r = lz_mont<1>(x, y, x, y);
    } else {
        Fq<2047, 32768> q;
#pragma unroll
        for (int k = 0; k < LN; k++) q.v[k] = x[k];
        if constexpr (op == 2) {
            const auto z = reduce(q);
#pragma unroll
            for (int k = 0; k < LN; k++) r.v[k] = z.v[k];
        } else {
            const auto z = squeeze(q);
#pragma unroll
            for (int k = 0; k < LN; k++) r.v[k] = z.v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < LN; k++) out[i * LN + k] = r.v[k];
}

}  // namespace

// host buffers of n x 14 int32 limbs each; returns 0 on success, -1 on a HIP error or bad op
extern "C" int cc_selftest_lazy(int op, size_t n, const int32_t* h_a, const int32_t* h_b, const int32_t* h_c,
                                const int32_t* h_d, int32_t* h_out) {
    if (op < 0 || op > 6 || !n) return -1;
    const size_t bytes = n * cc::lz::LN * sizeof(int32_t);
    int32_t* dv[5] = {};
    int rc = 0;
    for (int k = 0; k < 5 && !rc; k++)
        if (hipMalloc(&dv[k], bytes) != hipSuccess) rc = -1;
    const int32_t* hs[4] = {h_a, h_b ? h_b : h_a, h_c ? h_c : h_a, h_d ? h_d : h_a};
    for (int k = 0; k < 4 && !rc; k++)
        if (hipMemcpy(dv[k], hs[k], bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (!rc) {
        const dim3 g((unsigned)((n + 255) / 256)), b(256);
        if (op == 0) hipLaunchKernelGGL(k_lz_selftest<0>, g, b, 0, 0, n, dv[0], dv[1], dv[2], dv[3], dv[4]);
        else if (op == 1) hipLaunchKernelGGL(k_lz_selftest<1>, g, b, 0, 0, n, dv[0], dv[1], dv[2], dv[3], dv[4]);
        else if (op == 2) hipLaunchKernelGGL(k_lz_selftest<2>, g, b, 0, 0, n, dv[0], dv[1], dv[2], dv[3], dv[4]);
        else if (op == 3) hipLaunchKernelGGL(k_lz_selftest<3>, g, b, 0, 0, n, dv[0], dv[1], dv[2], dv[3], dv[4]);
        else if (op == 4) hipLaunchKernelGGL(k_lz_selftest<4>, g, b, 0, 0, n, dv[0], dv[1], dv[2], dv[3], dv[4]);
        else if (op == 5) hipLaunchKernelGGL(k_lz_selftest<5>, g, b, 0, 0, n, dv[0], dv[1], dv[2], dv[3], dv[4]);
        else hipLaunchKernelGGL(k_lz_selftest<6>, g, b, 0, 0, n, dv[0], dv[1], dv[2], dv[3], dv[4]);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -1;
    }
    if (!rc && hipMemcpy(h_out, dv[4], bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    for (int k = 0; k < 5; k++)
        if (dv[k]) (void)hipFree(dv[k]);
    return rc;
}

// ================================================================ cc_selftest_field
// The canonical 12 x 32 Fp of field.h (through the out-of-line fp_mul_call: this unit does not define
// CC_FP_INLINE, like every kernel that is not a pairing), its Fp2 helpers, and the scalar field of fr.h
// and codec.h, one row per lane, on raw rows taken as given (tests/test_gpu_field_edges.py compares each
// word with Python integers).  One instantiation per op, as above.
namespace {

enum FieldOp {
    FO_FP_ADD = 0, FO_FP_SUB, FO_FP_NEG, FO_FP_DBL, FO_FP_MUL, FO_FP_SQR, FO_FP_TO_MONT, FO_FP_FROM_MONT,
    FO_FP_RAW_REDUCE, FO_FP_INV, FO_F2_MUL, FO_F2_SQR, FO_F2_INV, FO_F2_MUL_XI,
    FO_FM_MUL, FO_FM_SUB, FO_FM_REDUCE_ONCE, FO_FM_FROM_U64, FO_FM_TO_CANON, FO_FR_MUL_CANON, FO_FR_INV_INT,
    FO_FM_INV, FO_RLC_DELTA_ABS, FO_FR_FROM_BE48, FO_COUNT
};

DEV void ld_row(cc::Fp& x, const uint32_t* p, size_t i) {
#pragma unroll
    for (int k = 0; k < cc::NL; k++) x.v[k] = p[i * cc::NL + k];
}
DEV void st_row(uint32_t* p, size_t i, const cc::Fp& x) {
#pragma unroll
    for (int k = 0; k < cc::NL; k++) p[i * cc::NL + k] = x.v[k];
}
DEV cc::Fm fm_of(const cc::Fp& x) {
    cc::Fm m;
#pragma unroll
    for (int k = 0; k < cc::NR; k++) m.v[k] = x.v[k];
    return m;
}
DEV void fm_to(cc::Fp& r, const cc::Fm& m) {
    cc::fp_zero(r);
#pragma unroll
    for (int k = 0; k < cc::NR; k++) r.v[k] = m.v[k];
}

// Fp2 ops: (a[i], b[i]) is one operand (real, imaginary), the second operand of f2_mul is row
// (i + 1) mod n, and the result goes to out rows i (real) and n + i (imaginary).
template <int op>
__global__ __launch_bounds__(256) void k_field_selftest(size_t n, const uint32_t* __restrict__ a,
                                                        const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
    using namespace cc;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp x, y, r;
    ld_row(x, a, i);
    ld_row(y, b, i);
    if constexpr (op >= FO_F2_MUL && op <= FO_F2_MUL_XI) {
        Fp2 u, v, w;
        u.a = x;
        u.b = y;
        if constexpr (op == FO_F2_MUL) {
            const size_t j = i + 1 < n ? i + 1 : 0;
            ld_row(v.a, a, j);
            ld_row(v.b, b, j);
            f2_mul(w, u, v);
        } else if constexpr (op == FO_F2_SQR) {
            f2_sqr(w, u);
        } else if constexpr (op == FO_F2_INV) {
            f2_inv(w, u);
        } else {
            f2_mul_xi(w, u);
        }
        st_row(out, i, w.a);
        st_row(out, n + i, w.b);
        return;
    } else if constexpr (op == FO_FP_ADD) {
        fp_add(r, x, y);
    } else if constexpr (op == FO_FP_SUB) {
        fp_sub(r, x, y);
    } else if constexpr (op == FO_FP_NEG) {
        fp_neg(r, x);
    } else if constexpr (op == FO_FP_DBL) {
        fp_dbl(r, x);
    } else if constexpr (op == FO_FP_MUL) {
        fp_mul(r, x, y);
    } else if constexpr (op == FO_FP_SQR) {
        fp_sqr(r, x);
    } else if constexpr (op == FO_FP_TO_MONT) {
        fp_to_mont(r, x);
    } else if constexpr (op == FO_FP_FROM_MONT) {
        fp_from_mont(r, x);
    } else if constexpr (op == FO_FP_RAW_REDUCE) {
        r = x;
        fp_raw_reduce(r);
    } else if constexpr (op == FO_FP_INV) {
        fp_inv(r, x);
    } else if constexpr (op == FO_FM_MUL) {
        fm_to(r, fm_mul_v(fm_of(x), fm_of(y)));
    } else if constexpr (op == FO_FM_SUB) {
        Fm d;
        fm_sub(d, fm_of(x), fm_of(y));
        fm_to(r, d);
    } else if constexpr (op == FO_FM_REDUCE_ONCE) {
        Fm d;
        fm_reduce_once(d, x.v);
        fm_to(r, d);
    } else if constexpr (op == FO_FM_FROM_U64) {
        fm_to(r, fm_from_u64((uint64_t)x.v[0] | ((uint64_t)x.v[1] << 32)));
    } else if constexpr (op == FO_FM_TO_CANON) {
        fm_to(r, fm_to_canon(fm_of(x)));
    } else if constexpr (op == FO_FR_MUL_CANON) {
        fp_zero(r);
        fr_mul_canon(r.v, x.v, y.v);
    } else if constexpr (op == FO_FR_INV_INT) {
        fp_zero(r);
        fr_inv_int(r.v, x.v);
    } else if constexpr (op == FO_FM_INV) {
        fm_to(r, fm_inv(fm_of(x)));
    } else if constexpr (op == FO_RLC_DELTA_ABS) {
        fp_zero(r);
        r.v[NR] = rlc_delta_abs(r.v, x.v) ? 1u : 0u;
    } else {
        Fr s;
        fr_from_be48(s, reinterpret_cast<const uint8_t*>(a + i * NL));
        fp_zero(r);
#pragma unroll
        for (int k = 0; k < NR; k++) r.v[k] = s.v[k];
    }
    st_row(out, i, r);
}

template <int op>
void launch_field(int want, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    if (want == op)
        hipLaunchKernelGGL(k_field_selftest<op>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, a, b, out);
    if constexpr (op + 1 < FO_COUNT) launch_field<op + 1>(want, n, a, b, out);
}

}  // namespace

// host buffers of n x 12 uint32 words (b may be NULL for a one-operand op; out holds 2n rows for the
// Fp2 ops 10..13); returns 0 on success, -1 on a HIP error or bad op
extern "C" int cc_selftest_field(int op, size_t n, const uint32_t* h_a, const uint32_t* h_b, uint32_t* h_out) {
    if (op < 0 || op >= FO_COUNT || !n || !h_a || !h_out) return -1;
    const size_t bytes = n * cc::NL * sizeof(uint32_t);
    const size_t obytes = op >= FO_F2_MUL && op <= FO_F2_MUL_XI ? 2 * bytes : bytes;
    uint32_t* dv[3] = {};
    int rc = 0;
    for (int k = 0; k < 3 && !rc; k++)
        if (hipMalloc(&dv[k], k == 2 ? obytes : bytes) != hipSuccess) rc = -1;
    if (!rc && hipMemcpy(dv[0], h_a, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (!rc && hipMemcpy(dv[1], h_b ? h_b : h_a, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (!rc) {
        launch_field<0>(op, n, dv[0], dv[1], dv[2]);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -1;
    }
    if (!rc && hipMemcpy(h_out, dv[2], obytes, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    for (int k = 0; k < 3; k++)
        if (dv[k]) (void)hipFree(dv[k]);
    return rc;
}
