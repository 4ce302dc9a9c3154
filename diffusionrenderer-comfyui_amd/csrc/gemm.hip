// bf16 GEMM for the DiT linears on gfx950 MFMA:  C[M,N] = epi(A[M,K] . W[N,K]^T)
//
// Both operands are K-contiguous (activations [tokens, K], nn.Linear weights [out, K]), so both tiles are
// staged by direct-to-LDS 16-byte loads (global_load_lds_dwordx4) and read back as 8-element K fragments.
//
// Tile 128x128x64, 256 threads = 4 waves (2 x 2), 64x64 per wave as 4x4 v_mfma_f32_16x16x32_bf16 tiles.
// The MFMA is issued as D = Wfrag x Afrag so a lane ends up with 4 CONSECUTIVE output features of one token
// (8-byte bf16 stores, and the gate / residual of the fused epilogue are read the same way).
//
// LDS: 2 stages x (A 16 KiB + W 16 KiB) = 64 KiB -> 2 workgroups per CU.  Rows are 128 B; the 16-byte chunk
// index is XOR-swizzled with (row>>1)&7, which makes every ds_read_b128 lane group hit 16 distinct 16-B slots
// of the 256-B bank row (conflict-free).  global_load_lds writes LDS lane-linearly, so the swizzle is applied
// to the per-lane SOURCE address and again on the read (cdna guide rule 21).
//
// Workgroup ids are remapped so that each XCD (own L2) walks a contiguous band of tiles, 8 tile-rows deep.
#include <stdlib.h>
#include "drn_common.h"
#include "drn_launchers.h"

#define BM 128
#define BN 128
#define BK 64
#define TILE_BYTES (BM * BK * 2)          // 16 KiB per operand per stage
#define STAGE_BYTES (2 * TILE_BYTES)

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                           bf16_t* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                                                           int64_t ldw, int64_t ldc, const bf16_t* __restrict__ gate,
                                                           const bf16_t* R, int64_t ldr, int64_t rpb,
                                                           float* __restrict__ part) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_BYTES];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    // ---- XCD-aware, grouped tile order
    const int tiles_m = (int)((M + BM - 1) / BM);
    const int tiles_n = (int)(N / BN);
    const int nwg = tiles_m * tiles_n;
    int pid;
    {
        const int bid = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int GROUP = 8;
    const int width = GROUP * tiles_n;
    const int group_id = pid / width;
    const int first_m = group_id * GROUP;
    const int gsz = min(tiles_m - first_m, GROUP);
    const int tm = first_m + (pid % width) % gsz;
    const int tn = (pid % width) / gsz;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

    // ---- staging: each wave copies 4 x 1 KiB pieces (8 rows x 128 B) of A and of W per K step
    const bf16_t* ga[4];
    const bf16_t* gw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 8 + (lane >> 3);          // tile row 0..127
        const int c = (lane & 7) ^ ((r >> 1) & 7);               // source chunk for LDS slot (lane&7)
        int64_t ra = m0 + r;
        if (ra > M - 1) ra = M - 1;                              // clamp: duplicates are never stored
        ga[i] = A + ra * lda + c * 8;
        gw[i] = W + (n0 + r) * ldw + c * 8;
    }
    auto stage = [&](int kt, int buf) {
        char* sa = smem + buf * STAGE_BYTES + wave * 4096;
        char* sw = sa + TILE_BYTES;
        const int64_t ko = (int64_t)kt * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((gptr_t)(ga[i] + ko), (lptr_t)(sa + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(gw[i] + ko), (lptr_t)(sw + i * 1024), 16, 0, 0);
        }
    };

    // ---- fragment read offsets (bytes within an operand tile), per k-substep ks: chunk = ks*4 + (lane>>4)
    const int fr = lane & 15, fq = lane >> 4;
    int offa[4][2], offw[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ra = wm * 64 + i * 16 + fr;
        const int rw = wn * 64 + i * 16 + fr;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int c = ks * 4 + fq;
            offa[i][ks] = ra * 128 + ((c ^ ((ra >> 1) & 7)) << 4);
            offw[i][ks] = rw * 128 + ((c ^ ((rw >> 1) & 7)) << 4);
        }
    }

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // split-K (gridDim.y > 1, small M: too few tiles to keep the CUs streaming weights): this workgroup multiplies K steps
    // [kbeg, kbeg + nk) and stores its fp32 partial tile; gemm_splitk_epilogue_kernel sums the partials and applies the epilogue
    const int nk = (int)(K / BK) / (int)gridDim.y;
    const int kbeg = (int)blockIdx.y * nk;
    stage(kbeg, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) stage(kbeg + kt + 1, (kt + 1) & 1);
        const char* sa = smem + (kt & 1) * STAGE_BYTES;
        const char* sw = sa + TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(sa + offa[i][ks]);
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const bf16x8_t*>(sw + offw[j][ks]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        }
    }

    if (part) {                                                   // split-K partial: fp32, [split][M][N]
        float* pp = part + (int64_t)blockIdx.y * M * N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t m = m0 + wm * 64 + i * 16 + fr;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<f32x4_t*>(pp + m * N + n0 + wn * 64 + j * 16 + fq * 4) = acc[i][j];
        }
        return;
    }
    // ---- epilogue: lane holds C[m][n..n+3], m = tile row (lane&15), n = 16 j + 4*(lane>>4) + r; column tiles j = 2p / 2p+1 are
    //      exchanged between lane rows fq = 2k / 2k+1 (v_permlane16_swap) so that a lane stores 16 B (see gemm256s.hip)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m_raw = m0 + wm * 64 + i * 16 + fr;
        const bool m_ok = m_raw < M;
        const int64_t m = m_ok ? m_raw : M - 1;
        const int64_t b = (EPI == DRN_EPI_GATE_RES) ? m / rpb : 0;
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
            uint2 o[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = 2 * jp + h;
                const int64_t n = n0 + wn * 64 + j * 16 + fq * 4;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = rbf(acc[i][j][r]);
                if (EPI == DRN_EPI_GELU) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = gelu_erf_fast(v[r]);
                } else if (EPI == DRN_EPI_GATE_RES) {
                    const uint2 g2 = *reinterpret_cast<const uint2*>(gate + b * N + n);
                    const uint2 r2 = *reinterpret_cast<const uint2*>(R + m * ldr + n);
                    const float g[4] = {bflo(g2.x), bfhi(g2.x), bflo(g2.y), bfhi(g2.y)};
                    const float x[4] = {bflo(r2.x), bfhi(r2.x), bflo(r2.y), bfhi(r2.y)};
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(g[r] * v[r]);
                }
                o[h].x = pack_bf2(v[0], v[1]);
                o[h].y = pack_bf2(v[2], v[3]);
            }
            const auto sx = __builtin_amdgcn_permlane16_swap(o[0].x, o[1].x, false, false);
            const auto sy = __builtin_amdgcn_permlane16_swap(o[0].y, o[1].y, false, false);
            const int64_t n8 = n0 + wn * 64 + jp * 32 + (fq & 1) * 16 + (fq >> 1) * 8;
            if (m_ok) *reinterpret_cast<uint4*>(C + m * ldc + n8) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
        }
    }
}

// sum of the split-K partials + the fused epilogue (same arithmetic as the in-kernel epilogue on the fp32 total)
template <int EPI>
__global__ __launch_bounds__(256) void gemm_splitk_epilogue_kernel(const float* __restrict__ part, int splits, bf16_t* C,
                                                                   int64_t M, int64_t N, int64_t ldc,
                                                                   const bf16_t* __restrict__ gate, const bf16_t* R,
                                                                   int64_t ldr, int64_t rpb) {
    const int64_t nq = N / 4, total = M * nq;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / nq, n = (i - m * nq) * 4;
        f32x4_t a = *reinterpret_cast<const f32x4_t*>(part + m * N + n);
        for (int s = 1; s < splits; ++s) a += *reinterpret_cast<const f32x4_t*>(part + ((int64_t)s * M + m) * N + n);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = rbf(a[r]);
        if (EPI == DRN_EPI_GELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = gelu_erf_fast(v[r]);
        } else if (EPI == DRN_EPI_GATE_RES) {
            const uint2 g2 = *reinterpret_cast<const uint2*>(gate + (m / rpb) * N + n);
            const uint2 r2 = *reinterpret_cast<const uint2*>(R + m * ldr + n);
            const float g[4] = {bflo(g2.x), bfhi(g2.x), bflo(g2.y), bfhi(g2.y)};
            const float x[4] = {bflo(r2.x), bfhi(r2.x), bflo(r2.y), bfhi(r2.y)};
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(g[r] * v[r]);
        }
        uint2 o;
        o.x = pack_bf2(v[0], v[1]);
        o.y = pack_bf2(v[2], v[3]);
        *reinterpret_cast<uint2*>(C + m * ldc + n) = o;
    }
}

// ---- host side.  gemm_plan.h decides which kernels a call launches on which rows (the cost model and every rule live there); this
// file holds the process's settings, runs the plans and reports them.
static GemmSettings& gemm_settings() { static GemmSettings s = gemm_settings_from_env(); return s; }
const GemmSettings& drn_gemm_settings() { return gemm_settings(); }
extern "C" void drn_gemm_force_tile(int tile) { gemm_settings().set_force(tile); }

// the one place that maps a kernel id of the plan to its launcher
static int gemm_launch_tile(int tile, const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                            int64_t ldw, int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr,
                            int64_t rows_per_batch, void* stream, const int64_t* blk) {
    if (tile == GEMM_K256)
        return drn_gemm256s_dispatch(A, W, C, M, N, K, lda, ldw, ldc, epilogue, gate, residual, ldr, rows_per_batch, stream, blk);
    if (tile == GEMM_K144)
        return drn_gemm144_dispatch(A, W, C, M, N, K, lda, ldw, ldc, epilogue, gate, residual, ldr, rows_per_batch, stream, blk);
    if (tile == GEMM_K384)
        return drn_gemm384_dispatch(A, W, C, M, N, K, lda, ldw, ldc, epilogue, gate, residual, ldr, rows_per_batch, stream, blk);
    if (tile == GEMM_KTALL)
        return drn_gemm_tall_dispatch(A, W, C, nullptr, M, N, K, lda, ldw, ldc, epilogue, gate, residual, ldr, rows_per_batch, 1, stream);
    const int64_t tiles = ((M + BM - 1) / BM) * (N / BN);
    DRN_CHECK_ARG(tiles < (1ll << 31));
    dim3 grid((unsigned)tiles), block(256);
    hipStream_t st = (hipStream_t)stream;
#define ARGS (const bf16_t*)A, (const bf16_t*)W, (bf16_t*)C, M, N, K, lda, ldw, ldc, (const bf16_t*)gate, \
             (const bf16_t*)residual, ldr, rows_per_batch, (float*)nullptr
    switch (epilogue) {
        case DRN_EPI_NONE: gemm_bf16_kernel<DRN_EPI_NONE><<<grid, block, 0, st>>>(ARGS); break;
        case DRN_EPI_GELU: gemm_bf16_kernel<DRN_EPI_GELU><<<grid, block, 0, st>>>(ARGS); break;
        case DRN_EPI_GATE_RES: gemm_bf16_kernel<DRN_EPI_GATE_RES><<<grid, block, 0, st>>>(ARGS); break;
        default: return DRN_EINVAL;
    }
#undef ARGS
    return drn_launch_status();
}

// the executor: the launches of the plan in order, each on its own rows of A, C and the residual, with its clip's gate row
static int gemm_impl(const void* A, const void* W, void* C, const GemmShape& p, const void* gate, const void* residual, void* stream) {
    DRN_CHECK_ARG(A && W && C && gemm_shape_ok(p));
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)C & 15) == 0);
    if (p.epilogue == DRN_EPI_GATE_RES) DRN_CHECK_ARG(gate && residual && ((uintptr_t)residual & 7) == 0);
    if (p.M == 0) return DRN_OK;
    if (p.epilogue < DRN_EPI_NONE || p.epilogue > DRN_EPI_GATE_RES) return DRN_EINVAL;
    const GemmSettings& s = gemm_settings();
    const int64_t Mb = p.clip_rows();
    GemmLaunch L;
    for (int64_t row = 0; row < p.M; row += L.rows) {
        DRN_CHECK_ARG(gemm_plan_next(s, p, row, &L) == DRN_OK);    // (a refusal comes at row 0: nothing has been launched)
        const int rc = gemm_launch_tile(L.kernel, (const bf16_t*)A + row * p.lda, W, (bf16_t*)C + row * p.ldc, L.rows, p.N, p.K, p.lda,
                                        p.ldw, p.ldc, p.epilogue,
                                        p.epilogue == DRN_EPI_GATE_RES ? (const bf16_t*)gate + row / Mb * p.N : gate,
                                        residual ? (const bf16_t*)residual + row * p.ldr : nullptr, p.ldr, L.rows_per_batch, stream, p.blk);
        if (rc != DRN_OK) return rc;
    }
    return DRN_OK;
}

extern "C" int drn_gemm_bf16(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                             int64_t ldw, int64_t ldc, int epilogue, const void* gate, const void* residual,
                             int64_t ldr, int64_t rows_per_batch, void* stream) {
    return gemm_impl(A, W, C, GemmShape{M, N, K, lda, ldw, ldc, ldr, epilogue, rows_per_batch, {62, 0, 62, 0}}, gate, residual, stream);
}

// drn_gemm_bf16 for a caller that measured the 384 x 256 tile faster than the plan without it on this product, in its own launch
// sequence and under the gate of profiles/gemm_plan.txt 3: the planner takes that tile if its other rules allow it (preconditions,
// whole rounds or fewer round-equivalents, DRN_GEMM384 / a forced tile), and plans as ever otherwise.  Not part of the C ABI.
int drn_gemm_bf16_measured384(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                              int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                              void* stream) {
    GemmShape p{M, N, K, lda, ldw, ldc, ldr, epilogue, rows_per_batch, {62, 0, 62, 0}};
    p.measured384 = true;
    return gemm_impl(A, W, C, p, gate, residual, stream);
}

// Same product with operands stored in column blocks ("planes"): logical A[m][k] lives at
// A + (k / a_block_cols) * a_block_stride + m * lda + k % a_block_cols, logical C[m][n] at
// C + (n / c_block_cols) * c_block_stride + m * ldc + n % c_block_cols (block_cols = 0: plain).  Block widths are powers of
// two, >= 64 for A and >= 256 for C.  Lets the sequence-parallel projections write the rank-major send buffer of the
// head <-> token all-to-all directly, and the output projection read the rank-major receive buffer.
extern "C" int drn_gemm_bf16_blocked(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                                     int64_t ldw, int64_t ldc, int epilogue, const void* gate, const void* residual,
                                     int64_t ldr, int64_t rows_per_batch, int64_t a_block_cols, int64_t a_block_stride,
                                     int64_t c_block_cols, int64_t c_block_stride, void* stream) {
    GemmShape p{M, N, K, lda, ldw, ldc, ldr, epilogue, rows_per_batch, {}};
    DRN_CHECK_ARG(gemm_shape_set_blocks(&p, a_block_cols, a_block_stride, c_block_cols, c_block_stride) == DRN_OK);
    return gemm_impl(A, W, C, p, gate, residual, stream);
}

// ---- the plan, without launching anything
extern "C" int drn_gemm_tile_choice(int64_t M, int64_t N) {
    return gemm_tile_echo(gemm_settings(), gemm_pick_tile(gemm_settings(), M, N));
}
extern "C" int drn_gemm_splitk_choice(int64_t M, int64_t N, int64_t K) {
    if (N % BN != 0 || K % BK != 0 || M <= 0) return 1;
    return gemm_plan_splitk(gemm_settings(), M, N, K, 0).splits;
}
// A plain [M, K] x [N, K] product of clips of rows_per_batch rows (<= 0 or >= M: one clip): the tile kernel of a clip's first launch
// (0 / 1 / 2 as drn_gemm_tile_choice, 5 = 384 x 256) and, in *main_rows, how many of the clip's rows it covers.  The few-token
// kernels are not reported here (drn_gemm_plan_describe does).
extern "C" int drn_gemm_plan_choice(int64_t M, int64_t N, int64_t K, int64_t rows_per_batch, int64_t* main_rows) {
    if (main_rows) *main_rows = 0;
    if (M <= 0 || N <= 0 || K <= 0 || N % BN != 0 || K % BK != 0) return DRN_EINVAL;
    const GemmShape p{M, N, K, K, K, N, 0, DRN_EPI_NONE, rows_per_batch, {62, 0, 62, 0}};
    int kernel = 0;
    const int64_t rows = gemm_plan_clip(gemm_settings(), p, p.clip_rows(), &kernel);
    if (main_rows) *main_rows = rows;
    return gemm_tile_echo(gemm_settings(), kernel);
}
// Every launch of the call drn_gemm_bf16 / drn_gemm_bf16_blocked / drn_gemm_bf16_splitk (splits > 1) would make of these arguments:
// up to `cap` records (kernel, first row, rows, rows_per_batch passed on) into `out`; returns their number, -1 where the call is refused.
// It walks the planner exactly as gemm_impl and splitk_slices do.
extern "C" int drn_gemm_plan_describe(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int epilogue,
                                      int64_t rows_per_batch, int64_t a_block_cols, int64_t c_block_cols, int splits, int64_t* out,
                                      int cap) {
    GemmShape p{M, N, K, lda, ldw, ldc, ldr, epilogue, rows_per_batch, {}};
    if (gemm_shape_set_blocks(&p, a_block_cols, 0, c_block_cols, 0) != DRN_OK || !gemm_shape_ok(p)) return -1;
    if (epilogue < DRN_EPI_NONE || epilogue > DRN_EPI_GATE_RES) return -1;
    const GemmSettings& s = gemm_settings();
    int n = 0;
    GemmLaunch L{0, 0, M, rows_per_batch};
    if (splits > 1) {
        if (p.blocked() || M <= 0 || splits > 64 || (K / BK) % splits != 0 || lda < K || ldc < N) return -1;
        if (((M + BM - 1) / BM) * (N / BN) >= 65536) return -1;       // splitk_slices' grid limit: the call is refused, so is its plan
        L.kernel = gemm_plan_splitk(s, p.clip_rows(), N, K, splits).kernel;
    }
    for (int64_t row = 0; row < M; row += L.rows, ++n) {
        if (splits <= 1 && gemm_plan_next(s, p, row, &L) != DRN_OK) return -1;
        if (out && n < cap) {
            const int64_t rec[4] = {L.kernel, L.row0, L.rows, L.rows_per_batch};
            for (int i = 0; i < 4; ++i) out[4 * n + i] = rec[i];
        }
    }
    return n;
}

// ---- split-K for small M (weight-streaming regime): `splits` workgroups per output tile, fp32 partials in `workspace`
extern "C" int64_t drn_gemm_splitk_workspace_bytes(int64_t M, int64_t N, int splits) {
    return splits > 1 ? (int64_t)splits * M * N * (int64_t)sizeof(float) : 0;
}

// the K slices of a split-K product: fp32 partials [splits][M][N] in `workspace`, nothing else (arguments validated by the callers)
static int splitk_slices(const void* A, const void* W, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                         int64_t rows_per_batch, int splits, void* workspace, void* stream) {
    const int64_t tiles = ((M + BM - 1) / BM) * (N / BN);
    DRN_CHECK_ARG(tiles < 65536);
    // which kernel computes the slices is a function of ONE clip's rows and the split count the caller got from
    // drn_gemm_splitk_choice for those rows (batch-invariant results).  Whether the 256-row slices take the weight ring is
    // drn_gemm256s_partial's own: it depends on what the device grants.
    const GemmSettings& s = gemm_settings();
    const int64_t Mb = (rows_per_batch > 0 && rows_per_batch < M && M % rows_per_batch == 0) ? rows_per_batch : M;
    switch (gemm_plan_splitk(s, Mb, N, K, splits).kernel) {
        case GEMM_KTALL:
            return drn_gemm_tall_dispatch(A, W, workspace, (float*)workspace, M, N, K, lda, ldw, N, DRN_EPI_NONE, nullptr, nullptr, 0,
                                          rows_per_batch, splits, stream);
        case GEMM_K256: return drn_gemm256s_partial(A, W, (float*)workspace, M, N, K, lda, ldw, splits, stream, !s.slices_avoid_ring);
    }
    gemm_bf16_kernel<DRN_EPI_NONE><<<dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, (hipStream_t)stream>>>(
        (const bf16_t*)A, (const bf16_t*)W, (bf16_t*)workspace, M, N, K, lda, ldw, N, nullptr, nullptr, 0, 1, (float*)workspace);
    return drn_launch_status();
}

// C_f32[M, N] = A . W^T as it leaves the accumulators (no rounding, no epilogue): ONE "slice" of the streamed 256 x 256 kernel's
// split-K form.  For products whose fp32 result feeds a softmax (the tokenizer's one-head spatial attention: 9216 x 9216 x 512 per
// frame).  M, N multiples of 256, K a multiple of 64; same K order per output element as every other tile kernel here.
extern "C" int drn_gemm_bf16_f32out(const void* A, const void* W, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                                    void* stream) {
    DRN_CHECK_ARG(A && W && C && M > 0 && N > 0 && K > 0 && M % 256 == 0 && N % 256 == 0 && K % BK == 0);
    DRN_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K);
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)C & 15) == 0);
    return drn_gemm256s_partial(A, W, C, M, N, K, lda, ldw, 1, stream, false);
}

// slices only: the caller sums them itself (drn_splitk_gate_res_ln_modulate folds the sum, the gated residual and the next
// LayerNorm into one pass).  Same slices, bit for bit, as drn_gemm_bf16_splitk computes.
extern "C" int drn_gemm_bf16_splitk_partials(const void* A, const void* W, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                                             int64_t rows_per_batch, int splits, void* workspace, void* stream) {
    DRN_CHECK_ARG(A && W && workspace && M > 0 && N > 0 && K > 0 && splits > 1 && splits <= 64);
    DRN_CHECK_ARG(K % BK == 0 && N % BN == 0 && (K / BK) % splits == 0);
    DRN_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K);
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
    return splitk_slices(A, W, M, N, K, lda, ldw, rows_per_batch, splits, workspace, stream);
}

// the reduce launch of a split-K product: sum of the fp32 slices [splits][M][N] + epilogue (arguments validated by the callers:
// drn_gemm_bf16_splitk below, drn_gemm_mxfp8_splitk in gemm_mx_tall.hip)
int drn_gemm_splitk_reduce(const void* workspace, int splits, void* C, int64_t M, int64_t N, int64_t ldc, int epilogue,
                           const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int64_t blocks = (M * (N / 4) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
#define EARGS (const float*)workspace, splits, (bf16_t*)C, M, N, ldc, (const bf16_t*)gate, (const bf16_t*)residual, ldr, rows_per_batch
    switch (epilogue) {
        case DRN_EPI_NONE: gemm_splitk_epilogue_kernel<DRN_EPI_NONE><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(EARGS); break;
        case DRN_EPI_GELU: gemm_splitk_epilogue_kernel<DRN_EPI_GELU><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(EARGS); break;
        default: gemm_splitk_epilogue_kernel<DRN_EPI_GATE_RES><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(EARGS); break;
    }
#undef EARGS
    return drn_launch_status();
}

extern "C" int drn_gemm_bf16_splitk(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                                    int64_t ldw, int64_t ldc, int epilogue, const void* gate, const void* residual,
                                    int64_t ldr, int64_t rows_per_batch, int splits, void* workspace, void* stream) {
    if (splits <= 1)
        return drn_gemm_bf16(A, W, C, M, N, K, lda, ldw, ldc, epilogue, gate, residual, ldr, rows_per_batch, stream);
    DRN_CHECK_ARG(A && W && C && workspace && M > 0 && N > 0 && K > 0 && splits <= 64);
    DRN_CHECK_ARG(K % BK == 0 && N % BN == 0 && (K / BK) % splits == 0);
    DRN_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && ldc % 8 == 0 && lda >= K && ldw >= K && ldc >= N);
    DRN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)C & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
    if (epilogue == DRN_EPI_GATE_RES)
        DRN_CHECK_ARG(gate && residual && ldr % 8 == 0 && ldr >= N && rows_per_batch > 0 && ((uintptr_t)residual & 7) == 0);
    if (epilogue < DRN_EPI_NONE || epilogue > DRN_EPI_GATE_RES) return DRN_EINVAL;
    {
        const int rc = splitk_slices(A, W, M, N, K, lda, ldw, rows_per_batch, splits, workspace, stream);
        if (rc != DRN_OK) return rc;
    }
    return drn_gemm_splitk_reduce(workspace, splits, C, M, N, ldc, epilogue, gate, residual, ldr, rows_per_batch, stream);
}

