// MXFP8 (OCP MX v1.0, e4m3fn elements + one E8M0 scale per 32 consecutive K elements) for the DiT block linears: the
// quantiser drn_mx_quant_bf16 and the block-scaled GEMM drn_gemm_mxfp8 on v_mfma_scale_f32_16x16x128_f8f6f4 (gfx950).
// Opt-in precision (HipDiT(precision="mxfp8")); the bf16 kernels are untouched.  Format rule, layouts and contract: drn.h.
//
// GEMM schedule: 256x256 output tile per 512-thread workgroup, K step 128 (= 128 bytes of a row, the bytes of the bf16 kernels'
// K step of 64), two LDS stages of [A 32 KiB | W 32 KiB | A scales 1 KiB | W scales 1 KiB], filled by 16-byte (data) and
// 4-byte (scales) global_load_lds.  One barrier per K step: the DMA of step k+1 flies while step k is computed.
// Data rows in LDS: 128 B, 16-byte slot s of row r holds global chunk s ^ ((r >> 1) & 7) (the swizzle of gemm256s: a 16-lane
// group reading one chunk of 16 consecutive rows touches all 64 banks once).
// Wave w owns A rows (w >> 2) * 128 .. +128 (8 row tiles mt) and W rows (w & 3) * 64 .. +64 (4 column tiles nt).
//
// Operand lane maps of the 16x16x128 scaled MFMA with 8-bit formats (checked with exact integer data, tests/test_mxfp8_gpu.py):
// lane l holds row l & 15, K elements 16 * (l >> 4) .. +15 in bytes 0..15 of its 8 VGPRs and 64 + 16 * (l >> 4) .. +15 in bytes
// 16..31 (the two K halves of the bf16 16x16x32 map, 16 bytes each: the fragment reads of gemm256s' two k-substeps), and the scale
// VGPR (op_sel byte 0) of lane l is that of row l & 15 and 32-block l >> 4.  (Lane q = l >> 4 holding K 32 q .. 32 q + 31
// instead gives the right products under the wrong scales: rel-L2 ~0.4 on random data.)  W is the first operand and A the second, as in gemm256s: the C/D map of
// the 16x16 shape (col = lane & 15, row = 4 * (lane >> 4) + r) then gives a lane 4 consecutive output COLUMNS of one row.
#include <type_traits>
#include "drn_common.h"
#include "drn_launchers.h"
#include "mx_quant.h"

namespace {

constexpr int MX_T = 256;                        // tile rows (M) and columns (N)
constexpr int MX_K = 128;                        // K step (elements = bytes)
constexpr int MX_DATA = MX_T * MX_K;             // 32 KiB per operand per stage
constexpr int MX_STAGE = 2 * MX_DATA + 2 * MX_T * 4;
constexpr int MX_A = 0, MX_W = MX_DATA, MX_SA = 2 * MX_DATA, MX_SW = 2 * MX_DATA + MX_T * 4;
constexpr int EPI_GELU_MX = 4;                   // internal: bf16(gelu(bf16(acc))) written as MXFP8 (C = elements [M, N], CS = scales)

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef const __attribute__((address_space(1))) void* mx_gptr_t;
typedef __attribute__((address_space(3))) void* mx_lptr_t;

// 4 lanes per 32-element block, 8 elements per lane: lane-group amax by two xor shuffles
__global__ __launch_bounds__(256) void mx_quant_kernel(const bf16_t* __restrict__ X, int64_t ldx, int chunks_per_row, int total,
                                                       uint8_t* __restrict__ Q, uint8_t* __restrict__ S, int64_t K) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool live = c < total;
    const int cc = live ? c : total - 1;
    const int row = cc / chunks_per_row, col = (cc - row * chunks_per_row) * 8;
    const uint4 v = *reinterpret_cast<const uint4*>(X + (int64_t)row * ldx + col);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) amax = max(amax, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
    const int e = mx_block_exp(amax);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);   // 2^-e, e in [-127, 120]: a normal float
    uint32_t q[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t h = (w[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
        q[i >> 2] |= f32_to_e4m3(__uint_as_float(h << 16) * inv) << ((i & 3) * 8);
    }
    if (live) {
        *reinterpret_cast<uint2*>(Q + (int64_t)row * K + col) = make_uint2(q[0], q[1]);
        if ((threadIdx.x & 3) == 0) S[(int64_t)row * (K / 32) + col / 32] = (uint8_t)(e + 127);
    }
}

// workgroup index (dispatch order; XCD = index & 7) -> tile: XCD-contiguous chunks, GROUP tile rows per L2 band (as gemm256s)
__device__ __forceinline__ void mx_tile_of(int bid, int nwg, int tiles_m, int tiles_n, int GROUP, int64_t& m0, int64_t& n0) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int width = GROUP * tiles_n;
    const int group_id = pid / width;
    const int first_m = group_id * GROUP;
    const int gsz = min(tiles_m - first_m, GROUP);
    m0 = (int64_t)(first_m + (pid % width) % gsz) * MX_T;
    n0 = (int64_t)((pid % width) / gsz) * MX_T;
}

// blocked operand layouts (drn_gemm_mxfp8_blocked, drn.h): A | SA in planes of a_cols columns (a plain A is ONE plane of K
// columns), C in planes of 1 << c_shift columns (shift 62 = plain).  The plain-layout kernel takes the empty form.
template <bool BLK> struct mx_blk_t {};
template <> struct mx_blk_t<true> {
    int64_t a_cols, a_stride, c_stride;
    int c_shift;
};
// where the next K step of A starts inside a row (BLK only): byte offset, and the bytes of the current plane's row still ahead
template <bool BLK> struct mx_astep_t {};
template <> struct mx_astep_t<true> { int64_t koff = 0, left = 0; };

// BLK = false is the plain-layout kernel: nothing of the blocked addressing reaches its code
template <int EPI, bool BLK = false>
__global__ __launch_bounds__(512, 1) void gemm_mx_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ SA,
                                                         const uint8_t* __restrict__ W, const uint8_t* __restrict__ SW,
                                                         bf16_t* C, int64_t M, int64_t N, int64_t K, int64_t ldc,
                                                         const bf16_t* __restrict__ gate, const bf16_t* R, int64_t ldr, int64_t rpb,
                                                         uint8_t* __restrict__ CS, const mx_blk_t<BLK> blk) {
    // the two stages as two LDS objects: the reads of one and the DMA into the other then provably do not alias, and the
    // compiler puts no vmcnt wait of its own in front of the fragment reads (one shared array: a vmcnt(0) before every step)
    __shared__ __attribute__((aligned(1024))) char lds0[MX_STAGE];
    __shared__ __attribute__((aligned(1024))) char lds1[MX_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int tiles_m = (int)((M + MX_T - 1) / MX_T), tiles_n = (int)(N / MX_T);
    int64_t m0, n0;
    mx_tile_of(blockIdx.x, tiles_m * tiles_n, tiles_m, tiles_n, 8, m0, n0);
    const int nk = (int)(K / MX_K);
    const int64_t sk = K / 32;                       // scale bytes per row

    // DMA sources: 4 pieces (8 rows each) of each operand per wave; one 4-byte scale piece (64 rows) per wave
    const uint8_t* srcA[4];
    const uint8_t* srcW[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int r = (wave * 4 + p) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        int64_t ra = m0 + r;
        if (ra > M - 1) ra = M - 1;
        if constexpr (BLK) srcA[p] = A + ra * blk.a_cols + c * 16;      // a plane's rows are a_cols bytes apart
        else srcA[p] = A + ra * K + c * 16;
        srcW[p] = W + (n0 + r) * K + c * 16;
    }
    const uint8_t* srcS;
    {
        const int r = (wave & 3) * 64 + lane;
        if (wave < 4) {
            int64_t ra = m0 + r;
            if (ra > M - 1) ra = M - 1;
            if constexpr (BLK) srcS = SA + ra * (blk.a_cols / 32);
            else srcS = SA + ra * sk;
        } else {
            srcS = SW + (n0 + r) * sk;
        }
    }
    const int s_dst = (wave < 4 ? MX_SA : MX_SW) + (wave & 3) * 256;

    // BLK: the K steps are requested in order (0, 1, 2, ...), so the byte offset of step kt inside an A row - plane * a_stride +
    // (k % a_cols) - is carried from call to call: a_cols % 128 == 0, so a step and its 4-byte scale piece (offset / 32 in SA,
    // whose planes are a_stride / 32 apart) never straddle a plane
    mx_astep_t<BLK> as;
    if constexpr (BLK) as.left = blk.a_cols;
    auto dma = [&](int kt, char* base) {
        int64_t ka;
        if constexpr (BLK) ka = as.koff; else ka = (int64_t)kt * MX_K;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            __builtin_amdgcn_global_load_lds((mx_gptr_t)(srcA[p] + ka), (mx_lptr_t)(base + MX_A + (wave * 4 + p) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((mx_gptr_t)(srcW[p] + (int64_t)kt * MX_K), (mx_lptr_t)(base + MX_W + (wave * 4 + p) * 1024), 16, 0, 0);
        }
        if constexpr (BLK) {
            __builtin_amdgcn_global_load_lds((mx_gptr_t)(srcS + (wave < 4 ? (ka >> 5) : (int64_t)kt * 4)), (mx_lptr_t)(base + s_dst), 4, 0, 0);
            as.koff += MX_K;
            as.left -= MX_K;
            if (as.left == 0) {
                as.koff += blk.a_stride - blk.a_cols;
                as.left = blk.a_cols;
            }
        } else {
            __builtin_amdgcn_global_load_lds((mx_gptr_t)(srcS + kt * 4), (mx_lptr_t)(base + s_dst), 4, 0, 0);
        }
    };

    // fragment read offsets: row fr of a 16-row tile, chunks fq and fq + 4 (K 16 fq .. +15 and 64 + 16 fq .. +15)
    const int fr = lane & 15, fq = lane >> 4;
    int offa0, offa1, offw0, offw1;
    {
        const int ra = wm * 128 + fr, rw = wn * 64 + fr;       // + 16 * mt / 16 * nt (does not change (r >> 1) & 7)
        offa0 = ra * 128 + ((fq ^ ((ra >> 1) & 7)) << 4);
        offa1 = ra * 128 + (((fq + 4) ^ ((ra >> 1) & 7)) << 4);
        offw0 = rw * 128 + ((fq ^ ((rw >> 1) & 7)) << 4);
        offw1 = rw * 128 + (((fq + 4) ^ ((rw >> 1) & 7)) << 4);
    }
    const int offsa = (wm * 128 + fr) * 4 + fq, offsw = (wn * 64 + fr) * 4 + fq;

    f32x4_t acc[8][4];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // one K step on stage ST (a literal)
    auto kstep = [&](int kt, auto ST) {
        constexpr int st = decltype(ST)::value;
        if (kt + 1 < nk) dma(kt + 1, st ? lds0 : lds1);
        const char* base = st ? lds1 : lds0;
        i32x8_t wf[4];
        int ws[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const uint4 lo = *reinterpret_cast<const uint4*>(base + MX_W + offw0 + nt * 2048);
            const uint4 hi = *reinterpret_cast<const uint4*>(base + MX_W + offw1 + nt * 2048);
            wf[nt] = (i32x8_t){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            ws[nt] = *reinterpret_cast<const uint8_t*>(base + MX_SW + offsw + nt * 64);
        }
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const uint4 lo = *reinterpret_cast<const uint4*>(base + MX_A + offa0 + mt * 2048);
            const uint4 hi = *reinterpret_cast<const uint4*>(base + MX_A + offa1 + mt * 2048);
            const i32x8_t af = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            const int as = *reinterpret_cast<const uint8_t*>(base + MX_SA + offsa + mt * 64);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[nt], af, acc[mt][nt], 0, 0, 0, ws[nt], 0, as);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // step k+1 has landed (this wave's pieces) ...
        __syncthreads();                                      // ... everyone's, and this stage is free for step k+2
    };
    dma(0, lds0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
        kstep(kt, std::integral_constant<int, 0>());
        if (kt + 1 < nk) kstep(kt + 1, std::integral_constant<int, 1>());
    }

    // epilogue: lane holds C[m0 + wm*128 + 16 mt + fr][n0 + wn*64 + 16 nt + 4 fq + r], r = 0..3 (8-byte stores)
    if (EPI == EPI_GELU_MX) {
        // the GELU epilogue, its bf16 result quantised here (drn.h; the bytes of drn_mx_quant_bf16 on what DRN_EPI_GELU writes): the
        // 32-column block j of a row is the tiles nt = 2 j, 2 j + 1 of the four lanes fq = 0..3 (lane ^ 16, lane ^ 32) with the
        // same fr, 8 values each.  The shuffles run for every row (a ragged last tile only masks the stores).
        uint8_t* CQ = reinterpret_cast<uint8_t*>(C);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int64_t m = m0 + wm * 128 + mt * 16 + fr;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                uint32_t w[2][2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = gelu_erf_fast(rbf(acc[mt][2 * j + t][r]));
                    w[t][0] = pack_bf2(v[0], v[1]);
                    w[t][1] = pack_bf2(v[2], v[3]);
                }
                uint32_t amax = max(max(mx_amax2(w[0][0]), mx_amax2(w[0][1])), max(mx_amax2(w[1][0]), mx_amax2(w[1][1])));
                amax = max(amax, (uint32_t)__shfl_xor((int)amax, 16, 64));
                amax = max(amax, (uint32_t)__shfl_xor((int)amax, 32, 64));
                const int e = mx_block_exp(amax);
                const float inv = mx_inv_scale(e);
                const int64_t n = n0 + wn * 64 + j * 32 + fq * 4;
                if (m < M) {
                    *reinterpret_cast<uint32_t*>(CQ + m * N + n) = mx_pack4(w[0][0], w[0][1], inv);
                    *reinterpret_cast<uint32_t*>(CQ + m * N + n + 16) = mx_pack4(w[1][0], w[1][1], inv);
                    if (fq == 0) CS[m * (N / 32) + (n >> 5)] = (uint8_t)(e + 127);
                }
            }
        }
        return;
    }
    if constexpr (BLK) C += (n0 >> blk.c_shift) * (blk.c_stride - ((int64_t)1 << blk.c_shift));   // the tile's plane (256 | plane width)
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        const int64_t m = m0 + wm * 128 + mt * 16 + fr;
        if (m >= M) continue;
        const int64_t b = (EPI == DRN_EPI_GATE_RES) ? m / rpb : 0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int64_t n = n0 + wn * 64 + nt * 16 + fq * 4;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rbf(acc[mt][nt][r]);
            if (EPI == DRN_EPI_GELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = gelu_erf_fast(v[r]);
            } else if (EPI == DRN_EPI_GATE_RES) {
                const uint2 gg = *reinterpret_cast<const uint2*>(gate + b * N + n);
                const uint2 rr = *reinterpret_cast<const uint2*>(R + m * ldr + n);
                const float g[4] = {bflo(gg.x), bfhi(gg.x), bflo(gg.y), bfhi(gg.y)};
                const float x[4] = {bflo(rr.x), bfhi(rr.x), bflo(rr.y), bfhi(rr.y)};
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(g[r] * v[r]);
            }
            *reinterpret_cast<uint2*>(C + m * ldc + n) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
        }
    }
}

template <int EPI>
int launch_mx_blocked(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N, int64_t K,
                      int64_t ldc, const void* gate, const void* R, int64_t ldr, int64_t rpb, const mx_blk_t<true>& blk, hipStream_t st) {
    const int64_t tiles = (M + MX_T - 1) / MX_T * (N / MX_T);
    gemm_mx_kernel<EPI, true><<<dim3((unsigned)tiles), dim3(512), 0, st>>>(
        (const uint8_t*)A, (const uint8_t*)SA, (const uint8_t*)W, (const uint8_t*)SW, (bf16_t*)C, M, N, K, ldc,
        (const bf16_t*)gate, (const bf16_t*)R, ldr, rpb, nullptr, blk);
    return drn_launch_status();
}

template <int EPI>
int launch_mx(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N, int64_t K, int64_t ldc,
              const void* gate, const void* R, int64_t ldr, int64_t rpb, hipStream_t st, void* CS = nullptr) {
    const int64_t tiles = (M + MX_T - 1) / MX_T * (N / MX_T);
    gemm_mx_kernel<EPI><<<dim3((unsigned)tiles), dim3(512), 0, st>>>(
        (const uint8_t*)A, (const uint8_t*)SA, (const uint8_t*)W, (const uint8_t*)SW, (bf16_t*)C, M, N, K, ldc,
        (const bf16_t*)gate, (const bf16_t*)R, ldr, rpb, (uint8_t*)CS, mx_blk_t<false>());
    return drn_launch_status();
}

}  // namespace

// the 256 x 256 kernel with the GELU -> MX epilogue (drn_gemm_mxfp8_gelu_mx in gemm_mx_tall.hip validates and dispatches)
int drn_gemm_mx_gelu_mx_launch(const void* A, const void* SA, const void* W, const void* SW, void* CQ, void* CS, int64_t M, int64_t N,
                               int64_t K, void* stream) {
    DRN_CHECK_ARG((M + MX_T - 1) / MX_T * (N / MX_T) < (1ll << 31));
    return launch_mx<EPI_GELU_MX>(A, SA, W, SW, CQ, M, N, K, N, nullptr, nullptr, 0, 1, (hipStream_t)stream, CS);
}

static int64_t g_mx_quant_calls = 0;       // launches enqueued by drn_mx_quant_bf16 (host-side; one host thread per process: drn.h)
extern "C" int64_t drn_mx_quant_calls(int reset) {
    const int64_t n = g_mx_quant_calls;
    if (reset) g_mx_quant_calls = 0;
    return n;
}

extern "C" int drn_mx_quant_bf16(const void* X, int64_t M, int64_t K, int64_t ldx, void* Q, void* scales, void* stream) {
    DRN_CHECK_ARG(X && Q && scales && M >= 1 && K >= 32 && K % 32 == 0 && ldx >= K && ldx % 8 == 0);
    DRN_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 7) == 0);
    // the kernel numbers its 8-element chunks in an int, the last workgroup's idle lanes included: total rounded up to 256 < 2^31
    DRN_CHECK_ARG(M <= ((1ll << 31) - 256) / (K / 8));
    const int total = (int)(M * (K / 8));
    ++g_mx_quant_calls;
    mx_quant_kernel<<<dim3((unsigned)(((int64_t)total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        (const bf16_t*)X, ldx, (int)(K / 8), total, (uint8_t*)Q, (uint8_t*)scales, K);
    return drn_launch_status();
}

extern "C" int drn_gemm_mxfp8(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N, int64_t K,
                              int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                              void* stream) {
    DRN_CHECK_ARG(A && SA && W && SW && C && M >= 1 && N >= MX_T && N % MX_T == 0 && K >= MX_K && K % MX_K == 0);
    DRN_CHECK_ARG(ldc >= N && ldc % 4 == 0 && ((uintptr_t)C & 7) == 0);
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)SA & 3) == 0 && ((uintptr_t)SW & 3) == 0);
    DRN_CHECK_ARG((M + MX_T - 1) / MX_T * (N / MX_T) < (1ll << 31));
    hipStream_t st = (hipStream_t)stream;
    switch (epilogue) {
        case DRN_EPI_NONE: return launch_mx<DRN_EPI_NONE>(A, SA, W, SW, C, M, N, K, ldc, nullptr, nullptr, 0, 1, st);
        case DRN_EPI_GELU: return launch_mx<DRN_EPI_GELU>(A, SA, W, SW, C, M, N, K, ldc, nullptr, nullptr, 0, 1, st);
        case DRN_EPI_GATE_RES: {
            const int64_t rpb = rows_per_batch > 0 ? rows_per_batch : M;
            DRN_CHECK_ARG(gate && residual && ldr >= N && ldr % 4 == 0 && ((uintptr_t)residual & 7) == 0 && ((uintptr_t)gate & 7) == 0);
            return launch_mx<DRN_EPI_GATE_RES>(A, SA, W, SW, C, M, N, K, ldc, gate, residual, ldr, rpb, st);
        }
        default: return DRN_EINVAL;
    }
}

// drn_gemm_mxfp8 with A | SA and / or C stored in column planes (drn.h): always the 256 x 256 kernel above
extern "C" int drn_gemm_mxfp8_blocked(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N,
                                      int64_t K, int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr,
                                      int64_t rows_per_batch, int64_t a_block_cols, int64_t a_block_stride, int64_t c_block_cols,
                                      int64_t c_block_stride, void* stream) {
    DRN_CHECK_ARG(A && SA && W && SW && C && M >= 1 && N >= MX_T && N % MX_T == 0 && K >= MX_K && K % MX_K == 0);
    DRN_CHECK_ARG(ldc % 4 == 0 && ((uintptr_t)C & 7) == 0);
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)SA & 3) == 0 && ((uintptr_t)SW & 3) == 0);
    DRN_CHECK_ARG((M + MX_T - 1) / MX_T * (N / MX_T) < (1ll << 31));
    mx_blk_t<true> blk = {K, 0, 0, 62};
    if (a_block_cols) {
        DRN_CHECK_ARG(a_block_cols >= MX_K && a_block_cols % MX_K == 0 && K % a_block_cols == 0);
        DRN_CHECK_ARG(a_block_stride % 128 == 0 && a_block_stride / a_block_cols >= M);     // scale planes: a_block_stride / 32 apart
        blk.a_cols = a_block_cols;
        blk.a_stride = a_block_stride;
    }
    if (c_block_cols) {
        int sh = 0;
        while (sh < 40 && ((int64_t)1 << sh) < c_block_cols) ++sh;
        DRN_CHECK_ARG(((int64_t)1 << sh) == c_block_cols && sh >= 8 && N % c_block_cols == 0 && ldc >= c_block_cols);
        DRN_CHECK_ARG(c_block_stride % 4 == 0 && c_block_stride >= c_block_cols && (c_block_stride - c_block_cols) / ldc >= M - 1);
        blk.c_shift = sh;
        blk.c_stride = c_block_stride;
    } else {
        DRN_CHECK_ARG(ldc >= N);
    }
    hipStream_t st = (hipStream_t)stream;
    switch (epilogue) {
        case DRN_EPI_NONE: return launch_mx_blocked<DRN_EPI_NONE>(A, SA, W, SW, C, M, N, K, ldc, nullptr, nullptr, 0, 1, blk, st);
        case DRN_EPI_GELU: return launch_mx_blocked<DRN_EPI_GELU>(A, SA, W, SW, C, M, N, K, ldc, nullptr, nullptr, 0, 1, blk, st);
        case DRN_EPI_GATE_RES: {
            const int64_t rpb = rows_per_batch > 0 ? rows_per_batch : M;
            DRN_CHECK_ARG(gate && residual && ldr >= N && ldr % 4 == 0 && ((uintptr_t)residual & 7) == 0 && ((uintptr_t)gate & 7) == 0);
            return launch_mx_blocked<DRN_EPI_GATE_RES>(A, SA, W, SW, C, M, N, K, ldc, gate, residual, ldr, rpb, blk, st);
        }
        default: return DRN_EINVAL;
    }
}
