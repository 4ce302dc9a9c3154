// Few-token MXFP8 linears (one clip of 256 .. 1024 rows: BASELINE configs 1 and 2): C = epi(dequant(A) . dequant(W)^T) with the
// operands, format and lane maps of drn_gemm_mxfp8 (gemm_mx.hip, drn.h) and the decomposition of gemm_tall.hip.
//
// drn_gemm_mxfp8 has one tile (256 x 256, whole K): at 256 rows a block linear is 16 - 64 workgroups on 256 CUs, and the product
// is a weight stream.  Here a workgroup owns a tile of one clip's rows x a narrow column band, over the whole K or over one of
// `splits` K slices (gridDim.y), so that column tiles x slices cover half to all of the CUs:
//   shape 1: 128 rows x 128 columns, 4 stages of [A 16 KiB | W 16 KiB | scales 1 KiB]       = 132 KiB of LDS
//   shape 0: 256 rows x  64 columns, 3 stages of [A 32 KiB | W  8 KiB | scales 1.25 KiB]    = 123.75 KiB
// (the bf16 kernel's 5 / 4 stages plus the scale blocks would take 165 KiB: one stage fewer each.)  A K step is 128 elements =
// 128 bytes of a row: the LDS rows, the 1 KiB DMA pieces (8 rows) and the chunk ^ ((row >> 1) & 7) swizzle on the source
// address are those of gemm_tall.hip; the scales of a K step are 4 bytes per row, one 4-byte global_load_lds per 64 rows,
// issued by the first (TM + TN) / 64 waves.
// Ring: the stages are filled by global_load_lds NSTAGE - 1 K steps ahead; stage k is waited for with a counted vmcnt (the
// younger stages stay in flight), a raw s_barrier publishes it and frees stage k - 1, which the DMA of step k + NSTAGE - 1
// refills.  One barrier per K step, no __syncthreads() (its fence would drain the DMA queue).  The waves that also load scales
// have one more DMA per stage in their queue, so the K loop exists twice, once per wait count, selected by a wave-uniform branch.
//
// 8 waves, wave tile 64 rows x 32 columns = 4 x 2 tiles of v_mfma_scale_f32_16x16x128_f8f6f4 (W first operand, A second: a lane
// holds 4 consecutive columns of one row): 12 ds_read_b128 + 6 ds_read_u8 + 8 MFMAs per K step.
// splits == 1: the epilogues of gemm_mx_kernel, rounding where it rounds.  splits > 1: the raw fp32 accumulators go to the
// workspace as [splits][M][N], the layout of the bf16 split-K slices, so gemm_splitk_epilogue_kernel (gemm.hip) and
// drn_splitk_gate_res_ln_modulate consume them unchanged.  The reduction stays at the launch boundary.
#include <stdlib.h>
#include <type_traits>
#include "drn_common.h"
#include "drn_launchers.h"
#include "mx_quant.h"

namespace {

constexpr int MXT_K = 128;                 // K step (elements = bytes)
constexpr int EPI_PARTIAL = 3;             // internal: fp32 slice [blockIdx.y][M][N] to the workspace
constexpr int EPI_GELU_MX = 4;             // internal: bf16(gelu(bf16(acc))) written as MXFP8 (Cv = elements [M, N], CS = scales)
#ifndef MX_TALL_SHAPE_DEFAULT
#define MX_TALL_SHAPE_DEFAULT 1            // 0: 256 x 64 (3 stages), 1: 128 x 128 (4 stages); DRN_MX_TALL_SHAPE overrides
#endif

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

template <int EPI, int TM, int TN, int NSTAGE>
__global__ __launch_bounds__(512, 1) void gemm_mx_tall_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ SA,
                                                              const uint8_t* __restrict__ W, const uint8_t* __restrict__ SW,
                                                              void* Cv, int64_t M, int64_t N, int64_t K, int64_t ldc,
                                                              const bf16_t* __restrict__ gate, const bf16_t* R, int64_t ldr,
                                                              int64_t rpb, uint8_t* __restrict__ CS) {
    constexpr int A_BYTES = TM * MXT_K, W_BYTES = TN * MXT_K, S_OFF = A_BYTES + W_BYTES;
    constexpr int STAGE_BYTES = S_OFF + (TM + TN) * 4;
    constexpr int WN = TN / 32;                // waves across the columns (8 / WN down the rows), wave tile 64 x 32
    constexpr int PA = TM / 64, PW = TN / 64;  // 1 KiB pieces (8 rows x 128 B) of A / W per wave and K step
    constexpr int NSP = (TM + TN) / 64;        // waves that load a 4-byte scale piece (64 rows) per K step
    static_assert((TM / 64) * (TN / 32) == 8 && PA >= 1 && PW >= 1 && NSP <= 8 && TM % 64 == 0, "8 waves of 64 x 32");
    extern __shared__ __attribute__((aligned(1024))) char smem[];     // NSTAGE * STAGE_BYTES, the ONLY LDS object
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // tile: all column tiles of one row tile are neighbours in dispatch order - they share the A panel in L2
    const int tiles_n = (int)(N / TN);
    const int tm = (int)(blockIdx.x / tiles_n), tn = (int)(blockIdx.x % tiles_n);
    const int64_t m0 = (int64_t)tm * TM, n0 = (int64_t)tn * TN;
    const int64_t sk = K / 32;                 // scale bytes per row (of the whole K)
    int64_t Ks = K;
    if (EPI == EPI_PARTIAL) {
        Ks = K / gridDim.y;
        A += (int64_t)blockIdx.y * Ks;
        W += (int64_t)blockIdx.y * Ks;
        SA += (int64_t)blockIdx.y * (Ks / 32);
        SW += (int64_t)blockIdx.y * (Ks / 32);
    }
    const int nk = (int)(Ks / MXT_K);

    // ---- DMA sources: this wave's PA pieces of A (rows 8 PA w ..), PW pieces of W (rows 8 PW w ..), and one scale piece
    const uint8_t* a_base = A + (m0 + wave * (8 * PA)) * K;
    const uint8_t* w_base = W + (n0 + wave * (8 * PW)) * K;
    uint32_t voffa[PA], voffw[PW];
    {
        const int rl = lane >> 3;                                   // row inside a piece
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int r = wave * (8 * PA) + p * 8 + rl;             // row inside the tile (the swizzle needs the full row)
            const int c = (lane & 7) ^ ((r >> 1) & 7);
            voffa[p] = (uint32_t)((p * 8 + rl) * K + c * 16);
        }
#pragma unroll
        for (int p = 0; p < PW; ++p) {
            const int r = wave * (8 * PW) + p * 8 + rl;
            const int c = (lane & 7) ^ ((r >> 1) & 7);
            voffw[p] = (uint32_t)((p * 8 + rl) * K + c * 16);
        }
    }
    const uint8_t* s_src;                                           // row 64 w + lane of [A rows | W rows]
    {
        const int r = (wave < NSP ? wave : 0) * 64 + lane;
        s_src = r < TM ? SA + (m0 + r) * sk : SW + (n0 + (r - TM)) * sk;
    }
    const int dma_a = wave * (PA * 1024), dma_w = A_BYTES + wave * (PW * 1024), dma_s = S_OFF + wave * 256;

    // ---- fragment read offsets inside a stage: row fr of a 16-row tile, chunks fq and fq + 4 (K 16 fq .. +15 and 64 + 16 fq .. +15)
    const int fr = lane & 15, fq = lane >> 4;
    int offa[4][2], offw[2][2], offsa[4], offsw[2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int r = wm * 64 + mt * 16 + fr;
        offa[mt][0] = r * 128 + ((fq ^ ((r >> 1) & 7)) << 4);
        offa[mt][1] = r * 128 + (((fq + 4) ^ ((r >> 1) & 7)) << 4);
        offsa[mt] = S_OFF + r * 4 + fq;
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int r = wn * 32 + nt * 16 + fr;
        offw[nt][0] = A_BYTES + r * 128 + ((fq ^ ((r >> 1) & 7)) << 4);
        offw[nt][1] = A_BYTES + r * 128 + (((fq + 4) ^ ((r >> 1) & 7)) << 4);
        offsw[nt] = S_OFF + TM * 4 + r * 4 + fq;
    }

    f32x4_t acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // the K loop for a wave that loads scales (SC = 1: PA + PW + 1 DMAs per stage in its queue) or does not (SC = 0)
    auto kloop = [&](auto SC) {
        constexpr int sc = decltype(SC)::value;
        constexpr int PER_STAGE = PA + PW + sc;
        auto stage = [&](int kt, int s) {
            char* sa_ = smem + s * STAGE_BYTES;
            const int64_t kb_ = (int64_t)kt * MXT_K;
#pragma unroll
            for (int p = 0; p < PA; ++p)
                __builtin_amdgcn_global_load_lds((gptr_t)(a_base + kb_ + voffa[p]), (lptr_t)(sa_ + dma_a + p * 1024), 16, 0, 0);
#pragma unroll
            for (int p = 0; p < PW; ++p)
                __builtin_amdgcn_global_load_lds((gptr_t)(w_base + kb_ + voffw[p]), (lptr_t)(sa_ + dma_w + p * 1024), 16, 0, 0);
            if (sc) __builtin_amdgcn_global_load_lds((gptr_t)(s_src + kt * 4), (lptr_t)(sa_ + dma_s), 4, 0, 0);
        };
        // prologue: K steps 0 .. NSTAGE - 2 (past the end the last step is re-requested into a dead stage: uniform wait counts)
#pragma unroll
        for (int i = 0; i < NSTAGE - 1; ++i) stage(min(i, nk - 1), i);
        int scur = 0, sreq = NSTAGE - 1;                              // stage of K step kt; stage that step kt + NSTAGE - 1 refills
        for (int kt = 0; kt < nk; ++kt) {
            // own pieces of stage kt have landed (the NSTAGE - 2 younger stages may fly)
            asm volatile("s_waitcnt vmcnt(%0)" :: "i"((NSTAGE - 2) * PER_STAGE) : "memory");
            __builtin_amdgcn_s_barrier();                             // stage kt visible; every wave is done reading stage kt - 1
            __builtin_amdgcn_sched_barrier(0);
            stage(min(kt + NSTAGE - 1, nk - 1), sreq);                // refill the stage of step kt - 1
            const char* st = smem + scur * STAGE_BYTES;
            scur = scur == NSTAGE - 1 ? 0 : scur + 1;
            sreq = sreq == NSTAGE - 1 ? 0 : sreq + 1;
            // the fragments are read as ext-vector values: read as uint4 structs the compiler cannot tell them from the in-flight
            // DMA writes and puts a vmcnt(0) in front of the reads, which drains the ring every K step (check the ISA after edits)
            i32x8_t wf[2];
            int ws[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const u32x4_t lo = *reinterpret_cast<const u32x4_t*>(st + offw[nt][0]);
                const u32x4_t hi = *reinterpret_cast<const u32x4_t*>(st + offw[nt][1]);
                wf[nt] = (i32x8_t){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
                ws[nt] = *reinterpret_cast<const uint8_t*>(st + offsw[nt]);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const u32x4_t lo = *reinterpret_cast<const u32x4_t*>(st + offa[mt][0]);
                const u32x4_t hi = *reinterpret_cast<const u32x4_t*>(st + offa[mt][1]);
                const i32x8_t af = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
                const int as = *reinterpret_cast<const uint8_t*>(st + offsa[mt]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[nt], af, acc[mt][nt], 0, 0, 0, ws[nt], 0, as);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the re-requests: nothing may land after exit
    };
    if (wave < NSP) kloop(std::integral_constant<int, 1>());
    else kloop(std::integral_constant<int, 0>());

    // ---- epilogue: a lane holds columns n .. n + 3 of row m
    if (EPI == EPI_GELU_MX) {
        // the wave's 32 columns are ONE MX block per row: tiles nt = 0, 1 of the four lanes fq = 0..3 (lane ^ 16, lane ^ 32) with
        // the same fr.  The bf16 result of the GELU epilogue, quantised as drn_mx_quant_bf16 would (gemm_mx.hip, drn.h).
        uint8_t* CQ = reinterpret_cast<uint8_t*>(Cv);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int64_t m = m0 + wm * 64 + mt * 16 + fr;
            uint32_t w[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = gelu_erf_fast(rbf(acc[mt][t][r]));
                w[t][0] = pack_bf2(v[0], v[1]);
                w[t][1] = pack_bf2(v[2], v[3]);
            }
            uint32_t amax = max(max(mx_amax2(w[0][0]), mx_amax2(w[0][1])), max(mx_amax2(w[1][0]), mx_amax2(w[1][1])));
            amax = max(amax, (uint32_t)__shfl_xor((int)amax, 16, 64));
            amax = max(amax, (uint32_t)__shfl_xor((int)amax, 32, 64));
            const int e = mx_block_exp(amax);
            const float inv = mx_inv_scale(e);
            const int64_t n = n0 + wn * 32 + fq * 4;
            *reinterpret_cast<uint32_t*>(CQ + m * N + n) = mx_pack4(w[0][0], w[0][1], inv);
            *reinterpret_cast<uint32_t*>(CQ + m * N + n + 16) = mx_pack4(w[1][0], w[1][1], inv);
            if (fq == 0) CS[m * (N / 32) + (n >> 5)] = (uint8_t)(e + 127);
        }
        return;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int64_t m = m0 + wm * 64 + mt * 16 + fr;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t n = n0 + wn * 32 + nt * 16 + fq * 4;
            if (EPI == EPI_PARTIAL) {
                float* part = reinterpret_cast<float*>(Cv) + (int64_t)blockIdx.y * M * N;
                *reinterpret_cast<f32x4_t*>(part + m * N + n) = acc[mt][nt];
                continue;
            }
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rbf(acc[mt][nt][r]);
            if (EPI == DRN_EPI_GELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = gelu_erf_fast(v[r]);
            } else if (EPI == DRN_EPI_GATE_RES) {
                const int64_t b = (int64_t)((uint32_t)m / (uint32_t)rpb);
                const uint2 g2 = *reinterpret_cast<const uint2*>(gate + b * N + n);
                const uint2 r2 = *reinterpret_cast<const uint2*>(R + m * ldr + n);
                const float g[4] = {bflo(g2.x), bfhi(g2.x), bflo(g2.y), bfhi(g2.y)};
                const float x[4] = {bflo(r2.x), bfhi(r2.x), bflo(r2.y), bfhi(r2.y)};
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(g[r] * v[r]);
            }
            *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(Cv) + m * ldc + n) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
        }
    }
}

struct mx_args {
    const void *A, *SA, *W, *SW;
    void* C;
    int64_t M, N, K, ldc;
    const void *gate, *residual;
    int64_t ldr, rpb;
    int splits;
    hipStream_t st;
    void* CS;                          // EPI_GELU_MX: the scale bytes (C = the elements)
};

template <int EPI, int TM, int TN, int NSTAGE>
int launch_shape(const mx_args& a) {
    constexpr int LDS = NSTAGE * ((TM + TN) * MXT_K + (TM + TN) * 4);
    static_assert(LDS <= 160 * 1024, "LDS budget of a gfx950 CU");
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_mx_tall_kernel<EPI, TM, TN, NSTAGE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const int64_t tiles = (a.M / TM) * (a.N / TN);
    gemm_mx_tall_kernel<EPI, TM, TN, NSTAGE><<<dim3((unsigned)tiles, (unsigned)a.splits), dim3(512), LDS, a.st>>>(
        (const uint8_t*)a.A, (const uint8_t*)a.SA, (const uint8_t*)a.W, (const uint8_t*)a.SW, a.C, a.M, a.N, a.K, a.ldc,
        (const bf16_t*)a.gate, (const bf16_t*)a.residual, a.ldr, a.rpb, (uint8_t*)a.CS);
    return drn_launch_status();
}

int g_shape = -1;                      // -1: DRN_MX_TALL_SHAPE or the built-in default
int g_small_m = -1;                    // -1: DRN_MX_SMALL_M or on

int tall_shape() {
    static int env = -1;
    if (env < 0) {
        const char* e = getenv("DRN_MX_TALL_SHAPE");
        env = e ? (e[0] == '1' ? 1 : 0) : MX_TALL_SHAPE_DEFAULT;
    }
    return g_shape >= 0 ? g_shape : env;
}

int small_m_on() {
    if (g_small_m < 0) {
        const char* e = getenv("DRN_MX_SMALL_M");
        g_small_m = (e && e[0] == '0') ? 0 : 1;
    }
    return g_small_m;
}

template <int EPI>
int launch(const mx_args& a) {
    if (tall_shape()) return launch_shape<EPI, 128, 128, 4>(a);
    return launch_shape<EPI, 256, 64, 3>(a);
}

// the contract of both split entry points (drn.h); nothing is launched when it fails
bool shape_ok(int64_t M, int64_t N, int64_t K, int64_t rpb, int splits) {
    if (M <= 0 || M % 256 != 0 || N <= 0 || N % 256 != 0 || K <= 0 || K % MXT_K != 0) return false;
    if (splits < 1 || splits > 64 || (K / MXT_K) % splits != 0) return false;
    const int64_t Mb = (rpb > 0 && rpb < M && M % rpb == 0) ? rpb : M;
    if (Mb > 1024) return false;
    if (M >= (1ll << 31) || (M / 128) * (N / 64) >= (1ll << 31)) return false;
    return 33 * K < (1ll << 32);                                     // 32-bit lane offsets inside a wave's rows
}

}  // namespace

extern "C" int drn_gemm_mxfp8_force_small_m(int on) {
    const int was = small_m_on();
    if (on >= 0) g_small_m = on ? 1 : 0;
    return was;
}

extern "C" int drn_gemm_mxfp8_tall_force_shape(int shape) {
    const int was = g_shape;
    g_shape = shape < 0 ? -1 : (shape ? 1 : 0);
    return was;
}

// Which kernel computes an [M, N, K] MXFP8 product of ONE clip (M = the clip's rows), and with how many K slices.  0: not a
// few-token shape (drn_gemm_mxfp8).  Decomposition first: where the 256 x 256 tiles of drn_gemm_mxfp8 already cover 3/4 of the
// 256 CUs (M = 1024: q|k|v 192 tiles, MLP-up 256) that kernel takes in fewer bytes per output and wins (measured: 83 against
// 91 us, 87 against 119 us).  Else M N / 16 384 column tiles (either shape) x the largest power-of-two slice count that keeps
// tiles x slices <= 256 (one round of the CUs, more than half of them busy) with at least 8 K steps per slice (two fills of the
// 4-stage ring: below that the prologue is the loop).  A pure function of (M, N, K) and the hook.
extern "C" int drn_gemm_mxfp8_splitk_choice(int64_t M, int64_t N, int64_t K) {
    if (!small_m_on() || M <= 0 || M > 1024 || M % 256 != 0 || N <= 0 || N % 256 != 0 || K <= 0 || K % MXT_K != 0) return 0;
    if (33 * K >= (1ll << 32)) return 0;
    if ((M / 256) * (N / 256) >= 192) return 0;
    const int64_t tiles = M * N / 16384, nk = K / MXT_K;
    int best = 1;
    for (int s = 2; s <= 64; s *= 2)
        if (tiles * s <= 256 && nk % s == 0 && nk / s >= 8) best = s;
    return best;
}

extern "C" int drn_gemm_mxfp8_splitk_partials(const void* A, const void* SA, const void* W, const void* SW, int64_t M, int64_t N,
                                              int64_t K, int64_t rows_per_batch, int splits, void* workspace, void* stream) {
    DRN_CHECK_ARG(A && SA && W && SW && workspace && splits > 1 && shape_ok(M, N, K, rows_per_batch, splits));
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)SA & 3) == 0 && ((uintptr_t)SW & 3) == 0);
    DRN_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
    const mx_args a = {A, SA, W, SW, workspace, M, N, K, N, nullptr, nullptr, 0, M, splits, (hipStream_t)stream, nullptr};
    return launch<EPI_PARTIAL>(a);
}

extern "C" int drn_gemm_mxfp8_splitk(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N,
                                     int64_t K, int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr,
                                     int64_t rows_per_batch, int splits, void* workspace, void* stream) {
    DRN_CHECK_ARG(A && SA && W && SW && C && shape_ok(M, N, K, rows_per_batch, splits));
    DRN_CHECK_ARG(ldc >= N && ldc % 4 == 0 && ((uintptr_t)C & 7) == 0);
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)SA & 3) == 0 && ((uintptr_t)SW & 3) == 0);
    DRN_CHECK_ARG(epilogue >= DRN_EPI_NONE && epilogue <= DRN_EPI_GATE_RES);
    const int64_t rpb = (rows_per_batch > 0 && rows_per_batch <= M) ? rows_per_batch : M;
    if (epilogue == DRN_EPI_GATE_RES)
        DRN_CHECK_ARG(gate && residual && ldr >= N && ldr % 4 == 0 && ((uintptr_t)residual & 7) == 0 && ((uintptr_t)gate & 7) == 0);
    if (splits > 1) {
        DRN_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0);
        const mx_args a = {A, SA, W, SW, workspace, M, N, K, N, nullptr, nullptr, 0, M, splits, (hipStream_t)stream, nullptr};
        const int rc = launch<EPI_PARTIAL>(a);
        if (rc != DRN_OK) return rc;
        return drn_gemm_splitk_reduce(workspace, splits, C, M, N, ldc, epilogue, gate, residual, ldr, rpb, stream);
    }
    const mx_args a = {A, SA, W, SW, C, M, N, K, ldc, gate, residual, ldr, rpb, 1, (hipStream_t)stream, nullptr};
    switch (epilogue) {
        case DRN_EPI_NONE: return launch<DRN_EPI_NONE>(a);
        case DRN_EPI_GELU: return launch<DRN_EPI_GELU>(a);
        default: return launch<DRN_EPI_GATE_RES>(a);
    }
}

// MLP-up with the quantise launch folded in: CQ | CS = drn_mx_quant_bf16(what DRN_EPI_GELU writes), bit for bit (drn.h)
extern "C" int drn_gemm_mxfp8_gelu_mx(const void* A, const void* SA, const void* W, const void* SW, void* CQ, void* CS, int64_t M,
                                      int64_t N, int64_t K, int64_t rows_per_batch, void* stream) {
    DRN_CHECK_ARG(A && SA && W && SW && CQ && CS && M >= 1 && N >= 256 && N % 256 == 0 && K >= MXT_K && K % MXT_K == 0);
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)SA & 3) == 0 && ((uintptr_t)SW & 3) == 0);
    DRN_CHECK_ARG(((uintptr_t)CQ & 3) == 0);
    const int64_t rpb = (rows_per_batch > 0 && rows_per_batch <= M) ? rows_per_batch : M;
    const int64_t Mb = (rpb < M && M % rpb == 0) ? rpb : M;
    const int splits = drn_gemm_mxfp8_splitk_choice(Mb, N, K);
    if (splits == 0) return drn_gemm_mx_gelu_mx_launch(A, SA, W, SW, CQ, CS, M, N, K, stream);
    DRN_CHECK_ARG(splits == 1 && shape_ok(M, N, K, rpb, 1));          // sliced K: the GELU lives in the reduce launch, no MX form
    const mx_args a = {A, SA, W, SW, CQ, M, N, K, N, nullptr, nullptr, 0, rpb, 1, (hipStream_t)stream, CS};
    return launch<EPI_GELU_MX>(a);
}
