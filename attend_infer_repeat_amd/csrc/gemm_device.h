// Device-side pieces shared by the GEMM kernels (gemm_kernels.hip) and the fused LSTM / `what`-head kernels (lstm_kernels.hip):
// vector and address-space types, the bf16 pack / convert helpers, one 16-deep MFMA chunk, and the operand loaders.
#pragma once
#include "air_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
// explicit global address space: descriptors that travel through memory (grouped launch) would otherwise make every
// operand access a FLAT load with a 64-bit VGPR address (+100 VGPRs, half the occupancy)
typedef const float __attribute__((address_space(1))) *gcf;
typedef float __attribute__((address_space(1))) *gf;
typedef gf gf_t;
typedef const f32x4 __attribute__((address_space(1))) *gcf4;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef const u32x4 __attribute__((address_space(1))) *gcu4;
typedef const u32x2 __attribute__((address_space(1))) *gcu2;
typedef const unsigned short __attribute__((address_space(1))) *gch;
typedef unsigned short __attribute__((address_space(1))) *gh_t;
struct Gemm16Ptrs { const void *A16, *B16; void *C16; };

__device__ __forceinline__ unsigned pk_bf16(float lo, float hi) {
    const bf16x2 v = __builtin_convertvector((f32x2){lo, hi}, bf16x2);
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ unsigned short bf16_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

// bf16 operand mode (BASELINE config 5, "bf16 MFMA MLP path"): storage stays fp32; the four k-values a lane holds for a
// 16-deep chunk are rounded to bf16 (RNE, v_cvt_pk_bf16_f32) in registers and ONE v_mfma_f32_16x16x16_bf16 replaces the
// four v_mfma_f32_16x16x4_f32 -- same lane->k mapping (k = 4g..4g+3), fp32 accumulate.  1/8 of the MFMA issue cycles.
__device__ __forceinline__ s16x4 to_bf16x4(f32x4 v) {
    const bf16x2 lo = __builtin_convertvector((f32x2){v.x, v.y}, bf16x2);
    const bf16x2 hi = __builtin_convertvector((f32x2){v.z, v.w}, bf16x2);
    const u32x2 p = {__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
    return __builtin_bit_cast(s16x4, p);
}
template <int MT, int NT, bool BF>
__device__ __forceinline__ void mfma_chunk(f32x4 (&acc)[MT][NT], const f32x4 (&fa)[MT], const f32x4 (&fb)[NT]) {
    if (BF) {
        s16x4 ha[MT], hb[NT];
#pragma unroll
        for (int a = 0; a < MT; ++a) ha[a] = to_bf16x4(fa[a]);
#pragma unroll
        for (int b = 0; b < NT; ++b) hb[b] = to_bf16x4(fb[b]);
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ha[a], hb[b], acc[a][b], 0, 0, 0);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < NT; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a][j], fb[b][j], acc[a][b], 0, 0, 0);
    }
}

// element k..k+3 of a k-contiguous operand row (row-major [rows, K]); zero outside
__device__ __forceinline__ f32x4 ld_kcontig(gcf p, int ld, int row, bool row_ok, int k, int K, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row_ok && k < K) {
        gcf q = p + (size_t)row * ld + k;
        if (vec && k + 3 < K) {
            v = *(gcf4)q;
        } else {
            v.x = q[0];
            if (k + 1 < K) v.y = q[1];
            if (k + 2 < K) v.z = q[2];
            if (k + 3 < K) v.w = q[3];
        }
    }
    return v;
}
// rows k..k+3, fixed column, of a k-strided operand (row-major [K, cols]); zero outside
__device__ __forceinline__ f32x4 ld_kstrided(gcf p, int ld, int col, bool col_ok, int k, int K) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (col_ok && k < K) {
        gcf q = p + (size_t)k * ld + col;
        v.x = q[0];
        if (k + 1 < K) v.y = q[ld];
        if (k + 2 < K) v.z = q[2 * (size_t)ld];
        if (k + 3 < K) v.w = q[3 * (size_t)ld];
    }
    return v;
}

// Unmasked variants for chunks that lie fully inside K.  Rows / columns beyond the matrix are CLAMPED to a valid
// address instead of masked: they only feed accumulator rows / columns that are never stored.
__device__ __forceinline__ f32x4 ld_kcontig_full(gcf p, int ld, int row, int k, bool vec) {
    gcf q = p + (size_t)row * ld + k;
    if (vec) return *(gcf4)q;
    f32x4 v;
    v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
    return v;
}
__device__ __forceinline__ f32x4 ld_kstrided_full(gcf p, int ld, int col, int k) {
    gcf q = p + (size_t)k * ld + col;
    f32x4 v;
    v.x = q[0]; v.y = q[ld]; v.z = q[2 * (size_t)ld]; v.w = q[3 * (size_t)ld];
    return v;
}

// ---- bf16 data path: helpers of the 32-deep v_mfma_f32_16x16x32_bf16 loaders (gemm_wide16_body and the wide16 LSTM kernels)
__device__ __forceinline__ float bf16_to_f32(unsigned bits16) { return __uint_as_float(bits16 << 16); }
__device__ __forceinline__ u32x4 pk8(f32x4 lo, f32x4 hi) {
    return (u32x4){pk_bf16(lo.x, lo.y), pk_bf16(lo.z, lo.w), pk_bf16(hi.x, hi.y), pk_bf16(hi.z, hi.w)};
}
// tile t (0..3) of eight 4-wide bf16 rows w[0..7] (row j = k + j; w[j].x = columns 0,1, w[j].y = columns 2,3)
template <int T_>
__device__ __forceinline__ u32x4 tr16(const u32x2 (&w)[8]) {
    constexpr unsigned sel = (T_ & 1) ? 0x07060302u : 0x05040100u;     // v_perm_b32: {hi half | lo half} of (S0, S1)
    u32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned lo = (T_ < 2) ? w[2 * d].x : w[2 * d].y, hi = (T_ < 2) ? w[2 * d + 1].x : w[2 * d + 1].y;
        r[d] = __builtin_amdgcn_perm(hi, lo, sel);
    }
    return r;
}
template <int T_>
__device__ __forceinline__ u32x4 tr32(const f32x4 (&w)[8]) {
    return (u32x4){pk_bf16(w[0][T_], w[1][T_]), pk_bf16(w[2][T_], w[3][T_]), pk_bf16(w[4][T_], w[5][T_]), pk_bf16(w[6][T_], w[7][T_])};
}
