// MXFP8 self-attention for head_dim 128 on v_mfma_scale_f32_16x16x128_f8f6f4 (gfx950): drn_attention_mxfp8, its split-KV form and
// the V^T quantiser drn_mx_quant_vt.  Opt-in (HipDiT(attention_precision="mxfp8")); the bf16 bodies are untouched.  Formats: drn.h.
//
// Both products of flash attention run on the block-scaled MFMA with e4m3 operands; the online softmax is fp32.
// Workgroup = 8 waves x 32 queries (two 16-query tiles qt), key tile 128.  Lane l = (c = l & 15, g = l >> 4); the operand lane map
// of the instruction is the one gemm_mx.hip documents: a lane holds K elements 16 g .. +15 (bytes 0..15) and 64 + 16 g .. +15 (bytes
// 16..31) of row / column c, its scale VGPR is the one of row c and 32-block g.
//   S^T[key][q] = K . Q^T : head dim 128 is ONE K step.  A = K rows, B = Q (registers, 8 VGPRs per query tile).  MFMA t (0..7) of a
//                           key tile takes as row m the key (t < 4 ? 0 : 64) + 16 (m >> 2) + 4 (t & 3) + (m & 3), so by the C/D map
//                           (row 4 g + r) sacc[t][qt][r] is the score of query 16 qt + c with key 64 (t >> 2) + 16 g + 4 (t & 3) + r:
//                           the eight MFMAs leave lane (c, g) keys 16 g .. +15 and 64 + 16 g .. +15 in order.
//   O^T[d][q] += V^T . P^T: that is the B fragment of P^T in natural key order, so P goes from the score registers to four e4m3
//                           bytes per VGPR (v_cvt_pk_fp8_f32) and straight into the MFMA; A = V^T rows (d = 16 dt + c) read like K
//                           rows (V is stored transposed and quantised along the keys), scale blocks = the natural 32-key blocks.
//                           -> acc[dt][qt][r] = O^T[16 dt + 4 g + r][16 qt + c]
//   P = rne_e4m3(p 2^PEXP) under the fixed operand scale 2^-PEXP, p = exp2((s - m) scale log2e) with m the reference maximum of the
//   query: kept while the tile maximum stays within RESCALE_THR (log2 units) of it, else replaced by the tile maximum (decided per
//   query: a query's bits do not depend on its neighbours).  2^THR 2^PEXP = 256 <= 448.  The denominator is the sum of the
//   QUANTISED probabilities: one more MFMA per tile multiplies P^T by a fragment of ones.
// K / V^T tiles (16 KiB each) and their scale columns (512 B each) are double-buffered in LDS by global_load_lds; one barrier per
// tile.  LDS rows are 128 B; 16-byte slot s of row r holds chunk s ^ f(r): for K f(r) = 2 ((r >> 4) & 3) | ((r >> 1) & 1) (the 16 rows
// of one fragment read are {0..3} + 16 {0..3} + const), for V^T f(r) = (r >> 1) & 7 (16 consecutive rows): every 16-lane group of a
// ds_read_b128 touches all 64 banks once.  Keys past Sk: the K rows are clamped to the last one and their scores masked; V^T is
// zero-padded to a multiple of 128 keys by its producer.
#include <type_traits>
#include "drn_common.h"
#include "drn_launchers.h"
#include "mx_quant.h"

#ifndef ATTMX_RESCALE_THR
#define ATTMX_RESCALE_THR 4     // log2 units
#endif
#ifndef ATTMX_PEXP
#define ATTMX_PEXP 4
#endif
static_assert((1 << ATTMX_RESCALE_THR) * (1 << ATTMX_PEXP) <= 448, "P must stay inside e4m3");

namespace {

constexpr int QROWS = 256;                       // queries per workgroup
constexpr int KT = 128;                          // key tile
constexpr int ST_K = 0, ST_V = 16384, ST_KS = 32768, ST_VS = 32768 + 512, STAGE = 32768 + 1024;
constexpr int PSCALE = 127 - ATTMX_PEXP;         // E8M0 byte of 2^-PEXP

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

#define MFMA_MX(A, B, C, SA, SB) __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, C, 0, 0, 0, SA, 0, SB)

__device__ __forceinline__ i32x8_t join8(const uint4& lo, const uint4& hi) {
    return (i32x8_t){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// MX = true: the unsplit epilogue also writes the bf16 output row as MXFP8 (OQ / OS as drn_attention_bf16_mx; O may be NULL)
template <bool MX>
__global__ __launch_bounds__(512, 2) void attention_mx_kernel(
    const uint8_t* __restrict__ QQ, const uint8_t* __restrict__ QS, const uint8_t* __restrict__ KQ, const uint8_t* __restrict__ KS,
    const uint8_t* __restrict__ VT, const uint8_t* __restrict__ VS, bf16_t* __restrict__ O, int heads, int64_t Sq, int64_t Sk_total,
    int64_t q_bs, int64_t k_bs, int64_t Skp, int64_t ldo, int64_t bso, float scale_log2e, int nqb, int total, int nsplit,
    int64_t kv_chunk, float* __restrict__ Opart, float* __restrict__ MLpart, uint8_t* __restrict__ OQ, uint8_t* __restrict__ OS,
    int64_t mx_bs) {
    // two stages as two LDS objects (gemm_mx.hip: the reads of one and the DMA into the other then provably do not alias)
    __shared__ __attribute__((aligned(1024))) char lds0[STAGE];
    __shared__ __attribute__((aligned(1024))) char lds1[STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;

    int pid;
    {   // dispatch order -> XCD-contiguous chunks (as attention16.hip)
        const int bid = blockIdx.x;
        const int q = total >> 3, r = total & 7, xcd = bid & 7;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int qb = pid % nqb;
    const int rest = pid / nqb;
    const int split = rest % nsplit;
    const int bh = rest / nsplit;
    const int b = bh / heads, head = bh - b * heads;
    const int64_t q0 = (int64_t)qb * QROWS + wave * 32;
    const int64_t kv_begin = (int64_t)split * kv_chunk;
    const int64_t Sk = min(kv_chunk, Sk_total - kv_begin);
    const int64_t rowb = (int64_t)heads * 128, srow = (int64_t)heads * 4;      // bytes per Q / K row, per scale row
    const int64_t vsrow = Skp / 32;

    // ---- Q fragments (B operand) and their scales: rows past Sq repeat the last one (never stored)
    i32x8_t qf[2];
    int qsc[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        int64_t qrow = q0 + 16 * qt + c;
        if (qrow > Sq - 1) qrow = Sq - 1;
        const int64_t r = b * q_bs + qrow;
        const uint8_t* qp = QQ + r * rowb + (int64_t)head * 128 + 16 * g;
        qf[qt] = join8(*reinterpret_cast<const uint4*>(qp), *reinterpret_cast<const uint4*>(qp + 64));
        qsc[qt] = QS[r * srow + head * 4 + g];
    }

    const uint8_t* Kb = KQ + (b * k_bs + kv_begin) * rowb + (int64_t)head * 128;
    const uint8_t* KSb = KS + (b * k_bs + kv_begin) * srow + head * 4;
    const uint8_t* VTb = VT + ((int64_t)b * heads + head) * 128 * Skp + kv_begin;
    const uint8_t* VSb = VS + ((int64_t)b * heads + head) * 128 * vsrow + kv_begin / 32;

    // ---- staging: a 16 KiB tile is 16 pieces of 1 KiB (8 rows x 128 B); wave w copies pieces 2 w, 2 w + 1 of K and of V^T, waves
    //      0 / 1 the K scales and 2 / 3 the V scales (64 rows x 4 B each); the swizzle sits on the SOURCE address
    auto dma = [&](int t, char* base) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = 2 * wave + i;
            const int r = 8 * p + (lane >> 3), s = lane & 7;
            const int64_t key = min((int64_t)t * KT + r, Sk - 1);
            const int kch = s ^ ((((r >> 4) & 3) << 1) | ((r >> 1) & 1));
            const int vch = s ^ ((r >> 1) & 7);
            __builtin_amdgcn_global_load_lds((gptr_t)(Kb + key * rowb + kch * 16), (lptr_t)(base + ST_K + p * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(VTb + (int64_t)r * Skp + (int64_t)t * KT + vch * 16),
                                             (lptr_t)(base + ST_V + p * 1024), 16, 0, 0);
        }
        if (wave < 2) {
            const int64_t key = min((int64_t)t * KT + 64 * wave + lane, Sk - 1);
            __builtin_amdgcn_global_load_lds((gptr_t)(KSb + key * srow), (lptr_t)(base + ST_KS + wave * 256), 4, 0, 0);
        } else if (wave < 4) {
            const int d = 64 * (wave - 2) + lane;
            __builtin_amdgcn_global_load_lds((gptr_t)(VSb + (int64_t)d * vsrow + t * 4), (lptr_t)(base + ST_VS + (wave - 2) * 256), 4, 0, 0);
        }
    };

    // ---- fragment read offsets.  K: MFMA t reads row r0 + 64 (t >> 2) + 4 (t & 3), whose swizzle term is that of r0
    const int r0 = 16 * (c >> 2) + (c & 3);
    const int kfl = ((c >> 2) << 1) | ((c & 3) >> 1);
    const int koff0 = r0 * 128 + ((g ^ kfl) << 4), koff1 = r0 * 128 + (((g + 4) ^ kfl) << 4);
    const int ksoff = r0 * 4 + g;
    const int voff0 = c * 128 + ((g ^ (c >> 1)) << 4), voff1 = c * 128 + (((g + 4) ^ (c >> 1)) << 4);     // + dt * 2048
    const int vsoff = c * 4 + g;                                                                              // + dt * 64

    f32x4_t acc[8][2];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) acc[dt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t lacc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};      // ones . P^T: every row = the row sum
    i32x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = 0x38383838;                                  // e4m3 1.0
    asm volatile("" : "+v"(ones));
    float m_run[2] = {-INFINITY, -INFINITY}, m_thr[2] = {-INFINITY, -INFINITY}, mcs[2] = {0.f, 0.f};
    const float thr_raw = (float)ATTMX_RESCALE_THR / scale_log2e;                      // the threshold in raw score units
    const int nt = (int)((Sk + KT - 1) / KT);

    auto tile = [&](int t, auto ST) {
        constexpr int st = decltype(ST)::value;
        if (t + 1 < nt) dma(t + 1, st ? lds0 : lds1);
        const char* base = st ? lds1 : lds0;

        // ---- S^T = K . Q^T
        f32x4_t sacc[8][2];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            const int ro = 64 * (tt >> 2) + 4 * (tt & 3);
            const i32x8_t kf = join8(*reinterpret_cast<const uint4*>(base + ST_K + koff0 + ro * 128),
                                     *reinterpret_cast<const uint4*>(base + ST_K + koff1 + ro * 128));
            const int ksc = *reinterpret_cast<const uint8_t*>(base + ST_KS + ksoff + ro * 4);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) sacc[tt][qt] = MFMA_MX(kf, qf[qt], (f32x4_t{0.f, 0.f, 0.f, 0.f}), ksc, qsc[qt]);
        }
        if ((int64_t)(t + 1) * KT > Sk) {            // mask keys past Sk (last tile only)
            const int64_t kbase = (int64_t)t * KT + 16 * g;
#pragma unroll
            for (int tt = 0; tt < 8; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kbase + 64 * (tt >> 2) + 4 * (tt & 3) + r >= Sk) { sacc[tt][0][r] = -INFINITY; sacc[tt][1][r] = -INFINITY; }
        }

        // ---- online softmax: a query's 128 scores live in the 4 lanes (c, g = 0..3)
        float mx[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float m = sacc[0][qt][0];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, sacc[tt][qt][r]);
            uint32_t u = __float_as_uint(m);
            auto s0 = __builtin_amdgcn_permlane32_swap(u, u, false, false);        // lanes l ^ 32
            u = __float_as_uint(fmaxf(__uint_as_float(s0[0]), __uint_as_float(s0[1])));
            s0 = __builtin_amdgcn_permlane16_swap(u, u, false, false);             // lanes l ^ 16
            mx[qt] = fmaxf(__uint_as_float(s0[0]), __uint_as_float(s0[1]));
        }
        if (__any(mx[0] > m_thr[0] || mx[1] > m_thr[1])) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const bool up = mx[qt] > m_thr[qt];                                 // per query: its four lanes agree
                const float m_new = up ? mx[qt] : m_run[qt];
                const float alpha = up ? __builtin_amdgcn_exp2f((m_run[qt] - m_new) * scale_log2e) : 1.0f;
                m_run[qt] = m_new;
                m_thr[qt] = m_new + thr_raw;
                mcs[qt] = m_new * scale_log2e - (float)ATTMX_PEXP;
                lacc[qt] *= alpha;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) acc[dt][qt] *= alpha;
            }
        }
        i32x8_t pb[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const float mc = mcs[qt];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) {
                float p[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(sacc[tt][qt][r] * scale_log2e - mc);     // p 2^PEXP
                const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(p[0], p[1], 0, false);
                pb[qt][tt] = __builtin_amdgcn_cvt_pk_fp8_f32(p[2], p[3], lo, true);
            }
        }

        // ---- O^T += V^T . P^T, row sums += ones . P^T
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            const i32x8_t vf = join8(*reinterpret_cast<const uint4*>(base + ST_V + voff0 + dt * 2048),
                                     *reinterpret_cast<const uint4*>(base + ST_V + voff1 + dt * 2048));
            const int vsc = *reinterpret_cast<const uint8_t*>(base + ST_VS + vsoff + dt * 64);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) acc[dt][qt] = MFMA_MX(vf, pb[qt], acc[dt][qt], vsc, PSCALE);
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) lacc[qt] = MFMA_MX(ones, pb[qt], lacc[qt], 127, PSCALE);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // tile t + 1 has landed (this wave's pieces) ...
        __syncthreads();                                      // ... everyone's, and this stage is free for tile t + 2
    };
    dma(0, lds0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < nt; t += 2) {
        tile(t, std::integral_constant<int, 0>());
        if (t + 1 < nt) tile(t + 1, std::integral_constant<int, 1>());
    }

    // ---- epilogue: O[q][head * 128 + d] = O^T[d][q] / l   (or the un-normalised partial when the keys are split: the layout and
    //      the (m, l) pairs of the bf16 bodies, merged by the same combine pass)
    if (nsplit > 1) {
        const int nbatch = total / (nqb * heads * nsplit);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int64_t qrow = q0 + 16 * qt + c;
            if (qrow < Sq) {
                const int64_t rowid = ((int64_t)split * nbatch + b) * Sq + qrow;
                float* op = Opart + rowid * ((int64_t)heads * 128) + (int64_t)head * 128 + 4 * g;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) *reinterpret_cast<f32x4_t*>(op + 16 * dt) = acc[dt][qt];
                if (g == 0) {
                    float2* ml = reinterpret_cast<float2*>(MLpart) + rowid * heads + head;
                    *ml = make_float2(m_run[qt], lacc[qt][0]);
                }
            }
        }
        return;
    }
    // a lane holds d = 16 dt + 4 g + r of query row 16 qt + c: the 32-element block j of a row is the tiles dt = 2 j, 2 j + 1 of the
    // four lanes g = 0..3 (lane ^ 16, lane ^ 32).  The shuffles run for every row (rows past Sq only mask the stores).
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const float inv = 1.0f / lacc[qt][0];
        const int64_t qrow = q0 + 16 * qt + c;
        const bool live = qrow < Sq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t w[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                w[u][0] = pack_bf2(acc[2 * j + u][qt][0] * inv, acc[2 * j + u][qt][1] * inv);
                w[u][1] = pack_bf2(acc[2 * j + u][qt][2] * inv, acc[2 * j + u][qt][3] * inv);
            }
            if (O && live) {
                bf16_t* op = O + b * bso + qrow * ldo + (int64_t)head * 128 + 32 * j + 4 * g;
                *reinterpret_cast<uint2*>(op) = make_uint2(w[0][0], w[0][1]);
                *reinterpret_cast<uint2*>(op + 16) = make_uint2(w[1][0], w[1][1]);
            }
            if (MX) {
                uint32_t amax = max(max(mx_amax2(w[0][0]), mx_amax2(w[0][1])), max(mx_amax2(w[1][0]), mx_amax2(w[1][1])));
                amax = max(amax, (uint32_t)__shfl_xor((int)amax, 16, 64));
                amax = max(amax, (uint32_t)__shfl_xor((int)amax, 32, 64));
                const int e = mx_block_exp(amax);
                const float qinv = mx_inv_scale(e);
                if (live) {
                    const int64_t r = (b * mx_bs + qrow) * heads + head;
                    *reinterpret_cast<uint32_t*>(OQ + r * 128 + 32 * j + 4 * g) = mx_pack4(w[0][0], w[0][1], qinv);
                    *reinterpret_cast<uint32_t*>(OQ + r * 128 + 32 * j + 16 + 4 * g) = mx_pack4(w[1][0], w[1][1], qinv);
                    if (g == 0) OS[r * 4 + j] = (uint8_t)(e + 127);
                }
            }
        }
    }
}

// V [B][Sk][heads][128] bf16 (strided) -> V^T elements [B][heads][128][Skp] e4m3 + scales [B][heads][128][Skp / 32]: one workgroup
// transposes 128 keys x 128 d through LDS; a 32-key block of one (head, d) row is quantised by one thread (the rule of drn.h).
__global__ __launch_bounds__(256) void mx_quant_vt_kernel(const bf16_t* __restrict__ V, uint8_t* __restrict__ VT,
                                                          uint8_t* __restrict__ VS, int heads, int64_t Sk, int64_t Skp, int64_t ldv,
                                                          int64_t bsv) {
    __shared__ bf16_t T[128][130];               // [d][key], rows padded to 65 words
    const int tid = threadIdx.x;
    const int kt = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const bf16_t* Vb = V + b * bsv + (int64_t)head * 128;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = it * 256 + tid;
        const int key = idx >> 4, ch = idx & 15;
        const int64_t gk = (int64_t)kt * 128 + key;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);    // keys past Sk count as zeros
        if (gk < Sk) v = *reinterpret_cast<const uint4*>(Vb + gk * ldv + ch * 8);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) T[ch * 8 + i][key] = (bf16_t)((w[i >> 1] >> ((i & 1) * 16)) & 0xffffu);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int item = it * 256 + tid;
        const int d = item >> 2, kb = item & 3;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&T[d][kb * 32]);
        uint32_t w[16];
        uint32_t amax = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            w[i] = src[i];
            amax = max(amax, mx_amax2(w[i]));
        }
        const int e = mx_block_exp(amax);
        const float inv = mx_inv_scale(e);
        uint32_t q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = mx_pack4(w[2 * i], w[2 * i + 1], inv);
        const int64_t row = ((int64_t)b * heads + head) * 128 + d;
        uint8_t* dst = VT + row * Skp + (int64_t)kt * 128 + kb * 32;
        *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
        *reinterpret_cast<uint4*>(dst + 16) = make_uint4(q[4], q[5], q[6], q[7]);
        VS[row * (Skp / 32) + kt * 4 + kb] = (uint8_t)(e + 127);
    }
}

int attention_mx_launch(const void* qq, const void* qs, const void* kq, const void* ks, const void* vt, const void* vs, void* o, void* oq,
                        void* os, int batch, int heads, int64_t Sq, int64_t Sk, int64_t q_bs, int64_t k_bs, int64_t ldo, int64_t bso,
                        float scale, int nsplit, void* workspace, void* stream) {
    DRN_CHECK_ARG(qq && qs && kq && ks && vt && vs && (o || oq) && batch > 0 && heads > 0 && Sq >= 0 && Sk > 0 && nsplit >= 1);
    DRN_CHECK_ARG(scale > 0.f && q_bs >= 0 && k_bs >= 0 && (batch == 1 || (q_bs >= Sq && k_bs >= Sk)));
    DRN_CHECK_ARG(((uintptr_t)qq & 15) == 0 && ((uintptr_t)kq & 15) == 0 && ((uintptr_t)vt & 15) == 0);
    DRN_CHECK_ARG(((uintptr_t)qs & 3) == 0 && ((uintptr_t)ks & 3) == 0 && ((uintptr_t)vs & 3) == 0);
    DRN_CHECK_ARG(ldo % 8 == 0 && bso % 8 == 0 && ldo >= (int64_t)heads * 128 && ((uintptr_t)o & 15) == 0);
    AttnLaunch L;
    DRN_TRY(drn_attention_prologue(&L, oq, os, true, batch, heads, Sq, Sk, ldo, bso, scale, nsplit, workspace, QROWS, KT));
    if (Sq == 0) return DRN_OK;
    const int64_t Skp = (Sk + KT - 1) / KT * KT;
    hipStream_t st = (hipStream_t)stream;
    // (a launch whose keys are split writes fp32 partials: the MX epilogue is the combine kernel's)
    if (oq && L.nsplit == 1)
        attention_mx_kernel<true><<<dim3((unsigned)L.total), dim3(512), 0, st>>>(
            (const uint8_t*)qq, (const uint8_t*)qs, (const uint8_t*)kq, (const uint8_t*)ks, (const uint8_t*)vt, (const uint8_t*)vs,
            (bf16_t*)o, heads, Sq, Sk, q_bs, k_bs, Skp, ldo, bso, L.scale_log2e, (int)L.nqb, (int)L.total, L.nsplit, L.kv_chunk, L.opart,
            L.mlpart, (uint8_t*)oq, (uint8_t*)os, L.mx_bs);
    else
        attention_mx_kernel<false><<<dim3((unsigned)L.total), dim3(512), 0, st>>>(
            (const uint8_t*)qq, (const uint8_t*)qs, (const uint8_t*)kq, (const uint8_t*)ks, (const uint8_t*)vt, (const uint8_t*)vs,
            (bf16_t*)o, heads, Sq, Sk, q_bs, k_bs, Skp, ldo, bso, L.scale_log2e, (int)L.nqb, (int)L.total, L.nsplit, L.kv_chunk, L.opart,
            L.mlpart, nullptr, nullptr, 0);
    if (L.nsplit > 1) {
        DRN_TRY(drn_launch_status());                    // a failed partials launch: its code, and no combine pass behind it
        drn_attention_combine_launch(L.opart, L.mlpart, o, L.nsplit, batch, heads, Sq, ldo, bso, L.scale_log2e, oq, os, L.mx_bs, st);
    }
    return drn_launch_status();
}

}  // namespace

// Which self-attention sites of an engine with the switch on run on these kernels (host-only; drn.h).  Measured on one attention
// site of the 32-head model (tools/mxbench.py attn, producers counted) and on the whole step: slower at 256 tokens (one more
// launch in front of a 20 us kernel; cfg 1 4.72 -> 4.84 ms/step), equal at 1024, ahead from 2048 (-11 %; -24.5 % at 18 432).
static int g_attmx_force = 0;
extern "C" int drn_attention_mxfp8_force(int on) {
    const int was = g_attmx_force;
    if (on == 0 || on == 1) g_attmx_force = on;
    return was;
}
extern "C" int drn_attention_mxfp8_choice(int heads, int64_t S) {
    if (heads <= 0 || S <= 0) return 0;
    return (g_attmx_force || S >= 2048) ? 1 : 0;
}

// what the kernel does, for tests and emulations (host-only)
extern "C" int drn_attention_mxfp8_params(int* key_tile, float* rescale_thr, int* pexp) {
    DRN_CHECK_ARG(key_tile && rescale_thr && pexp);
    *key_tile = KT;
    *rescale_thr = (float)ATTMX_RESCALE_THR;
    *pexp = ATTMX_PEXP;
    return DRN_OK;
}

extern "C" int drn_mx_quant_vt(const void* v, void* vt, void* vs, int batch, int heads, int64_t Sk, int64_t ldv, int64_t bsv,
                               void* stream) {
    DRN_CHECK_ARG(v && vt && vs && batch > 0 && batch <= 65535 && heads > 0 && heads <= 65535 && Sk >= 1);
    DRN_CHECK_ARG(ldv >= (int64_t)heads * 128 && ldv % 8 == 0 && bsv % 8 == 0 && bsv >= 0);
    DRN_CHECK_ARG(((uintptr_t)v & 15) == 0 && ((uintptr_t)vt & 15) == 0 && ((uintptr_t)vs & 3) == 0);
    const int64_t Skp = (Sk + KT - 1) / KT * KT;
    DRN_CHECK_ARG(Skp / KT < (1ll << 31));
    mx_quant_vt_kernel<<<dim3((unsigned)(Skp / KT), (unsigned)heads, (unsigned)batch), dim3(256), 0, (hipStream_t)stream>>>(
        (const bf16_t*)v, (uint8_t*)vt, (uint8_t*)vs, heads, Sk, Skp, ldv, bsv);
    return drn_launch_status();
}

extern "C" int drn_attention_mxfp8(const void* qq, const void* qs, const void* kq, const void* ks, const void* vt, const void* vs,
                                   void* o, void* oq, void* os, int batch, int heads, int64_t Sq, int64_t Sk, int64_t q_bs,
                                   int64_t k_bs, int64_t ldo, int64_t bso, float scale, void* stream) {
    return attention_mx_launch(qq, qs, kq, ks, vt, vs, o, oq, os, batch, heads, Sq, Sk, q_bs, k_bs, ldo, bso, scale, 1, nullptr, stream);
}

extern "C" int drn_attention_splitkv_mxfp8(const void* qq, const void* qs, const void* kq, const void* ks, const void* vt,
                                           const void* vs, void* o, void* oq, void* os, int batch, int heads, int64_t Sq, int64_t Sk,
                                           int64_t q_bs, int64_t k_bs, int64_t ldo, int64_t bso, float scale, int nsplit,
                                           void* workspace, void* stream) {
    return attention_mx_launch(qq, qs, kq, ks, vt, vs, o, oq, os, batch, heads, Sq, Sk, q_bs, k_bs, ldo, bso, scale, nsplit, workspace,
                               stream);
}
