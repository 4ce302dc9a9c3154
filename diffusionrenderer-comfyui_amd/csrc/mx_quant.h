// MXFP8 quantisation rule shared by drn_mx_quant_bf16 (gemm_mx.hip) and the producers that write their bf16 result as MX
// directly (LayerNorm + modulate, the attention epilogue, the GELU epilogue of the MXFP8 GEMMs).  Format and rule: drn.h.
// A fused producer rounds to bf16 where its bf16-writing twin rounds and quantises THAT value: the bits of drn_mx_quant_bf16.
#pragma once
#include "drn_common.h"

// |v| <= 448, finite -> OCP e4m3fn bits, round to nearest even (integer arithmetic: the same bits as torch's conversion)
__device__ __forceinline__ uint32_t f32_to_e4m3(float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t sign = (u >> 24) & 0x80u;
    const uint32_t a = u & 0x7fffffffu;
    uint32_t r;
    if (a >= 0x3c800000u) {                                   // >= 2^-6: normal e4m3, 3 mantissa bits kept
        r = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
    } else {                                                  // subnormal e4m3: multiples of 2^-9 (8 * 2^-9 = the smallest normal)
        r = (uint32_t)__builtin_rintf(__uint_as_float(a) * 512.0f);
    }
    return r | sign;
}

// E8M0 exponent of a block from the bit pattern of its bf16 absolute maximum (finite): floor(log2(amax)) - 8, one more when the
// significand of amax is above 1.75 (so that amax / 2^e <= 448), clamped to [-127, 127]; an all-zero block gets -127.
__device__ __forceinline__ int mx_block_exp(uint32_t amax_bits) {
    if (amax_bits == 0) return -127;
    const int E = (int)(amax_bits >> 7), m = (int)(amax_bits & 0x7f);
    int e;
    if (E > 0) {
        e = E - 127 - 8 + (m > 96 ? 1 : 0);                   // 1 + m / 128 > 1.75
    } else {                                                  // bf16 subnormal: m * 2^-133
        const int p = 31 - __builtin_clz((unsigned)m);
        e = -133 + p - 8 + (4 * m > 7 * (1 << p) ? 1 : 0);
    }
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// 2^-e of a block exponent e in [-127, 127]: a normal float for e <= 126 (e = 127 needs amax >= 2^135: not a bf16 value)
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }

// |bits| of the larger of the two bf16 halves of a packed word
__device__ __forceinline__ uint32_t mx_amax2(uint32_t w) { return max(w & 0x7fffu, (w >> 16) & 0x7fffu); }

// two / four scaled values -> e4m3 bytes by v_cvt_pk_fp8_f32 (gfx950: OCP e4m3fn, round to nearest even; |v| <= 448 here by the
// block rule, so its saturation never acts): the bytes of f32_to_e4m3 at 1/2 instruction per element instead of ~20 - inside an
// epilogue that runs on a few CUs (attention at 256 tokens: 32 workgroups) the integer form cost more than the launch it saves.
// drn_mx_quant_bf16 keeps the integer form; tests/test_mxfp8_fused_gpu.py holds the two to the same bytes.
__device__ __forceinline__ uint32_t mx_pack2(uint32_t w, float inv) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(bflo(w) * inv, bfhi(w) * inv, 0, false) & 0xffffu;
}
// four bf16 values (two packed words) -> four e4m3 bytes under the block scale 2^-e
__device__ __forceinline__ uint32_t mx_pack4(uint32_t w0, uint32_t w1, float inv) {
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(w0) * inv, bfhi(w0) * inv, 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(bflo(w1) * inv, bfhi(w1) * inv, lo, true);
}
// the same from four fp32 values that are already bf16-exact (rounded through bf16 by their producer)
__device__ __forceinline__ uint32_t mx_pack4f(float a, float b, float c, float d, float inv) {
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c * inv, d * inv, lo, true);
}
// |bits| of a bf16-exact fp32 value as bf16 bits
__device__ __forceinline__ uint32_t mx_abs_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) >> 16; }
