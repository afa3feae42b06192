// mfma_tile.h — the device primitives every MFMA kernel file shares (conv3_mfma.hip, upconv_mfma.hip, head_loss.hip):
// the one MFMA shape of the library, the transposing LDS fragment read, and the 16-byte store pack.
#pragma once
#include "common.h"

typedef float __attribute__((ext_vector_type(2))) f32x2;
typedef unsigned __attribute__((ext_vector_type(2))) u32x2;
typedef unsigned __attribute__((ext_vector_type(4))) u32x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// D(16 x 16, fp32) += A(16 x 32) * B(32 x 16), bf16 operands: 8 k-values per lane, lane group g = lane >> 4 holds k = 8g .. 8g + 7
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// MFMA fragment of an operand whose K index is the STRIDED one in LDS ([k][16 channels], 32 B per k): two transposing reads
// (ds_read_b64_tr_b16), k +0..3 and +4..7 (128 B further) of this lane group's 8-deep run
__device__ __forceinline__ bf16x8 tr_frag(const char* base, int byteoff) {
    auto* p0 = (lds_bf16x4*)(base + byteoff);
    auto* p1 = (lds_bf16x4*)(base + byteoff + 128);
    bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p0);
    bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p1);
    return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// 16-byte store pack: two 8-byte results (a, b) per lane trade halves between 16-lane rows (v_permlane16_swap: the odd rows of
// a <-> the even rows of b).  Even rows end up with (a of this row, a of the row above), odd rows with (b of the row below, b of
// this row), as dwords {lo0, lo1, hi0, hi1}.  Which channels / voxels that makes is the caller's layout: see each use site.
__device__ __forceinline__ u32x4 swap_halves16(bf16x4 a, bf16x4 b) {
    u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
    u32x2 p0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
    u32x2 p1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
    return u32x4{p0[0], p1[0], p0[1], p1[1]};
}
