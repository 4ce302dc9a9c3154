// 384x256x64 bf16 GEMM at ONE wave per SIMD, streamed schedule:  C = epi(A[M,K] . W[N,K]^T), whole tiles only (tile kernel 5)
//
// Why: gemm256s_kernel is bound by operand ingest (one 1 KiB LDS-DMA piece per ~37 cycles per CU); pieces per
// FLOP depend only on the tile, (BM + BN) / (BM BN): 1/128 at 256 x 256, 1/153.6 here.  And 18 432 rows are 48 tiles of 384: the
// four block linears of the headline shape fill whole rounds of the 256 CUs, with no 144-row tail launch.
//
// Geometry.  256 threads = 4 waves, one per SIMD, 2 (wr: rows) x 2 (wc: columns).  The tile is two A halves of 192 rows (A0, A1)
// times two W halves of 128 output columns (W0, W1); a wave owns 96 x 64 of each of the four (A half, W half) pairs = 6 x 4 MFMA
// tiles (v_mfma_f32_16x16x32_bf16, D = Wfrag x Afrag as in gemm256s: a lane holds 4 consecutive columns of one row).
// LDS: 2 stages x (A0 A1: 2 x 24 KiB, W0 W1: 2 x 16 KiB) = 160 KiB, ONE __shared__ object; 128-B rows, 16-byte chunk ^ ((row >> 1) & 7),
// swizzle on the DMA source address (gemm256s_core.h).  A half-tile is 24 (A) or 16 (W) pieces of 1 KiB = 8 rows; wave w moves
// pieces 4 p + w: the swizzle term of a lane's row is then the same for every p, and a piece is addressed as a uniform half-tile
// base (an SGPR pair) + a 32-bit lane offset that already holds the piece's 32 p rows.
//
// Registers (one wave per execution unit: the unified file of 512, at most 256 architected + 256 accumulator registers).
// Accumulators: 2 x 6 x 2 x 4 tiles x 4 = 384, more than the 256 AGPRs: the MFMAs are asm statements that pin 64 tiles to AGPRs
// ("+a") and 32 tiles to VGPRs ("+v").  Left to itself hipcc spilled ~800 registers per lane.  With both k-substeps of a K step
// resident the fragments would be 112 more (A 6 x 2 x 4, W 2 buffers x 4 x 2 x 4: 496 of 512) and hipcc still spilled ~120 - so
// the K step runs as TWO half steps, k-substep 0 then 1, and only one k-substep's fragments are resident: A 24 + W 2 x 16 = 56.
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950, all three epilogues: VGPRs 256, AGPRs 256, scratch 0 bytes per lane, no
// VGPR or SGPR spill, occupancy 1 wave per SIMD; the loop (two K steps) is 384 MFMAs, 80 ds_read_b128, 40 DMA pieces, 10 barriers
// and no other vector instruction than 12 address adds.
//
// Schedule of a half step (stage S, k-substep ks), 4 groups of 24 MFMAs in one continuous stream - (A0,W0) (A0,W1) (A1,W1) (A1,W0) -
// fragments requested a group ahead into the register that just died (per output element the order stays ks ascending inside a
// K step, K steps ascending, fp32: the bits of gemm256s_kernel):
//     group 1 (order [mt][nt]): W1   -> the free W buffer                       (4 reads)
//     group 2 (order [mt][nt]): A1   -> af[mt] as its A0 entry dies             (6)
//     group 3 (order [nt][mt]): W0 of the NEXT half step -> the W1 buffer, entry nt as it dies   (4)
//     group 4 (order [mt][nt]): A0 of the next half step -> af[mt] as its A1 entry dies          (6)
// The two W buffers swap roles every half step.  A region is read twice (ks = 0, 1) and re-filled no sooner than two groups after
// its last read; the 20 pieces a wave requests per K step are spread 2 2 3 3 | 2 2 3 3 over the 8 groups:
//     first half of step k:   W1(k+1) in groups 1, 2   A1(k+1) in groups 3, 4    -> stage S ^ 1 (read last in the half step before k)
//     second half of step k:  W0(k+2) in groups 1, 2   A0(k+2) in groups 3, 4    -> stage S (read last in groups 3 / 4 of the first half)
// Every half-tile is requested 6 to 9 groups (2300+ matrix-pipe cycles) before its first read.  ONE counted wait in front of a
// hand-over barrier retires the half-tile whose first read follows; with the in-order queue per step [W1 A1 W0 A0] = [4 6 4 6]
// the YOUNGER pieces that may stay in flight are
//     after group 1 of the first half:   A1(k)   needed: W0(k+1) 4 + A0(k+1) 6 + this group's 2             = 12
//     after group 2 of the second half:  W0(k+1) needed: A0(k+1) 6 + this step's 4 + 6 + 4                  = 20
//     after group 3 of the second half:  A0(k+1) needed: this step's 4 + 6 + 4 + 3                          = 17
//     after group 4 of the second half:  W1(k+1) needed: A1(k+1) 6 + W0(k+2) 4 + A0(k+2) 6                  = 16
// A fifth barrier (no wait) after group 4 of the first half frees W0 / A0 of stage S; the other three group ends hand nothing
// over.  Requests past the end re-request the last K step into regions nobody reads any more, so the counts hold to the last
// step (nk >= 2).  No vmcnt(0) in the loop; the only vector-memory operations in it are the DMA pieces (stores follow the loop).
// The fragment reads are plain loads (hipcc counts lgkmcnt for them: nothing else in the loop uses that counter); the DMA pieces
// and the MFMAs are asm, so hipcc neither waits for a DMA nor moves an accumulator.
//
// Measured (MI355X, S = 18 432, interleaved with today's plan in one process; profiles/gemm384.txt): MLP-down 4 % faster, QKV and
// MLP-up within the old kernel's spread, out-proj a tie - the dispatcher takes this kernel for MLP-down only.
#include <stdlib.h>
#include "drn_common.h"
#include "drn_launchers.h"

#define G384_BM 384
#define G384_BN 256
#define G384_BK 64
#define G384_AH (192 * G384_BK * 2)                 // 24 KiB
#define G384_WH (128 * G384_BK * 2)                 // 16 KiB
#define G384_STAGE (2 * G384_AH + 2 * G384_WH)      // 80 KiB
#define G384_LDS (2 * G384_STAGE)                   // 160 KiB
#define G384_A(S, I) ((S) * G384_STAGE + (I) * G384_AH)
#define G384_W(S, J) ((S) * G384_STAGE + 2 * G384_AH + (J) * G384_WH)

typedef const __attribute__((address_space(1))) void* g384_gptr_t;
typedef __attribute__((address_space(3))) void* g384_lptr_t;

// workgroup index (dispatch order; XCD = index & 7) -> tile: XCD-contiguous chunks, GROUP tile rows per L2 band (tile_of of
// gemm256s_core.h with this tile's extents; bijective for every nwg)
static __device__ __forceinline__ void tile_of384(int bid, int nwg, int tiles_m, int tiles_n, int GROUP, int64_t& m0, int64_t& n0) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int width = GROUP * tiles_n;
    const int group_id = pid / width;
    const int first_m = group_id * GROUP;
    const int gsz = min(tiles_m - first_m, GROUP);
    m0 = (int64_t)(first_m + (pid % width) % gsz) * G384_BM;
    n0 = (int64_t)((pid % width) / gsz) * G384_BN;
}

#define FENCE() __builtin_amdgcn_sched_barrier(0)
// fragment of k-substep KS (32 of the K step's 64 columns = chunks 4 KS .. 4 KS + 3 of the row: offa[KS] = offa[0] ^ 64)
#define LDA(S, I, MT, KS) (*reinterpret_cast<const bf16x8_t*>(smem + G384_A(S, I) + offa[KS] + (MT) * 2048))
#define LDW(S, J, NT, KS) (*reinterpret_cast<const bf16x8_t*>(smem + G384_W(S, J) + offw[KS] + (NT) * 2048))
// One LDS-DMA piece: 64 lanes x 16 B from (uniform base + 32-bit lane offset) to the wave-uniform LDS address `dst`.  An asm
// statement, so that the address stays ONE SGPR pair + ONE VGPR (through the builtin hipcc kept a 64-bit lane pointer per piece)
// and hipcc's own wait counts never see it.  M0 is saved and restored around it; one wait state between the write of M0 and the DMA.
static __device__ __forceinline__ void g384_dma16(const char* sbase, uint32_t voff, uint32_t dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(dst) : "memory");
}
// piece P of this wave of A half I / W half J into stage S, from the uniform base BASE (that half-tile's rows at the K step wanted);
// the piece's 32 P rows are part of the lane offset (voffa[P], voffw[P]): no address arithmetic beside the MFMAs
#define DMA_A(I, P, BASE, S) g384_dma16(BASE, voffa[P], lds0 + G384_A(S, I) + (P) * 4096 + dma_off)
#define DMA_W(J, P, BASE, S) g384_dma16(BASE, voffw[P], lds0 + G384_W(S, J) + (P) * 4096 + dma_off)
// The MFMAs are asm statements so that the accumulators' register class is OURS: the tiles of (A0,W0), (A0,W1) and mt >= 2 of
// (A1,W1) live in AGPRs ("+a": 64 tiles = 256 registers, all there are), the other 32 tiles in VGPRs beside the fragments.  An
// accumulate chain needs no wait states, and the fragment operands come straight from ds_read destinations (plain loads: hipcc
// waits for them).
#define G384_IN_V(I, MT, J) ((I) == 1 && ((J) == 0 || (MT) < 2))
#define MM(I, MT, J, NT, WF)                                                                                           \
    do {                                                                                                               \
        if (G384_IN_V(I, MT, J))                                                                                       \
            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[I][MT][J][NT]) : "v"(WF[NT]), "v"(af[MT])); \
        else                                                                                                           \
            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[I][MT][J][NT]) : "v"(WF[NT]), "v"(af[MT])); \
    } while (0)
// a slot that ends the life of af[MT]: its four MFMAs, then the slot's share of the fragment requests and DMA
#define SLOT_M(I, J, MT, WF, WORK)                                                                                     \
    do {                                                                                                               \
        MM(I, MT, J, 0, WF); MM(I, MT, J, 1, WF); MM(I, MT, J, 2, WF); MM(I, MT, J, 3, WF);                            \
        WORK;                                                                                                          \
        FENCE();                                                                                                       \
    } while (0)
// a slot that ends the life of WF[NT]: its six MFMAs
#define SLOT_N(I, J, NT, WF, WORK)                                                                                     \
    do {                                                                                                               \
        MM(I, 0, J, NT, WF); MM(I, 1, J, NT, WF); MM(I, 2, J, NT, WF);                                                 \
        MM(I, 3, J, NT, WF); MM(I, 4, J, NT, WF); MM(I, 5, J, NT, WF);                                                 \
        WORK;                                                                                                          \
        FENCE();                                                                                                       \
    } while (0)
#define HANDOVER(VM)                                                                                                   \
    do {                                                                                                               \
        FENCE();                                                                                                       \
        asm volatile("s_waitcnt vmcnt(" #VM ")" ::: "memory");                                                         \
        __builtin_amdgcn_s_barrier();                                                                                  \
        FENCE();                                                                                                       \
    } while (0)
#define HANDOVER_B()                     /* nothing new to land: every wave's reads of the groups before are issued */     \
    do {                                                                                                               \
        FENCE();                                                                                                       \
        __builtin_amdgcn_s_barrier();                                                                                  \
        FENCE();                                                                                                       \
    } while (0)
#define HANDOVER_N() FENCE()             /* no region changes hands here */
// Half step (stage S, k-substep KS), W0 fragments in WA, A0 fragments in af; (SN, KSN) = the half step that follows.  DW(P) /
// DA(P): this half step's DMA pieces (4 W, 6 A); H1..H4: the hand-overs.  On exit af = A0 and WB = W0 of (SN, KSN).
#define HSTEP(S, KS, SN, KSN, WA, WB, DW, DA, H1, H2, H3, H4)                                                          \
    do {                                                                                                               \
        /* group 1 (A0,W0): W1 -> WB (free) */                                                                         \
        SLOT_M(0, 0, 0, WA, WB[0] = LDW(S, 1, 0, KS));                                                                 \
        SLOT_M(0, 0, 1, WA, WB[1] = LDW(S, 1, 1, KS));                                                                 \
        SLOT_M(0, 0, 2, WA, WB[2] = LDW(S, 1, 2, KS));                                                                 \
        SLOT_M(0, 0, 3, WA, WB[3] = LDW(S, 1, 3, KS));                                                                 \
        SLOT_M(0, 0, 4, WA, DW(0));                                                                                    \
        SLOT_M(0, 0, 5, WA, DW(1));                                                                                    \
        H1;                                                                                                            \
        /* group 2 (A0,W1): A1 -> af as its A0 entries die */                                                          \
        SLOT_M(0, 1, 0, WB, af[0] = LDA(S, 1, 0, KS));                                                                 \
        SLOT_M(0, 1, 1, WB, (af[1] = LDA(S, 1, 1, KS), DW(2)));                                                        \
        SLOT_M(0, 1, 2, WB, af[2] = LDA(S, 1, 2, KS));                                                                 \
        SLOT_M(0, 1, 3, WB, (af[3] = LDA(S, 1, 3, KS), DW(3)));                                                        \
        SLOT_M(0, 1, 4, WB, af[4] = LDA(S, 1, 4, KS));                                                                 \
        SLOT_M(0, 1, 5, WB, af[5] = LDA(S, 1, 5, KS));                                                                 \
        H2;                                                                                                            \
        /* group 3 (A1,W1), order [nt][mt]: W0 of the next half step -> WB as its W1 entries die */                    \
        SLOT_N(1, 1, 0, WB, (WB[0] = LDW(SN, 0, 0, KSN), DA(0)));                                                      \
        SLOT_N(1, 1, 1, WB, (WB[1] = LDW(SN, 0, 1, KSN), DA(1)));                                                      \
        SLOT_N(1, 1, 2, WB, (WB[2] = LDW(SN, 0, 2, KSN), DA(2)));                                                      \
        SLOT_N(1, 1, 3, WB, WB[3] = LDW(SN, 0, 3, KSN));                                                               \
        H3;                                                                                                            \
        /* group 4 (A1,W0): A0 of the next half step -> af as its A1 entries die */                                    \
        SLOT_M(1, 0, 0, WA, af[0] = LDA(SN, 0, 0, KSN));                                                               \
        SLOT_M(1, 0, 1, WA, (af[1] = LDA(SN, 0, 1, KSN), DA(3)));                                                      \
        SLOT_M(1, 0, 2, WA, af[2] = LDA(SN, 0, 2, KSN));                                                               \
        SLOT_M(1, 0, 3, WA, (af[3] = LDA(SN, 0, 3, KSN), DA(4)));                                                      \
        SLOT_M(1, 0, 4, WA, af[4] = LDA(SN, 0, 4, KSN));                                                               \
        SLOT_M(1, 0, 5, WA, (af[5] = LDA(SN, 0, 5, KSN), DA(5)));                                                      \
        H4;                                                                                                            \
    } while (0)
// K step k in stage S: its first half requests W1 / A1 of step k + 1 (K index KD1) into stage S ^ 1, its second half W0 / A0 of
// step k + 2 (KD2) into stage S (their regions were read for the last time in groups 3 / 4 of the first half)
#define KSTEP(S, KD1, KD2)                                                                                             \
    do {                                                                                                               \
        HSTEP(S, 0, S, 1, wx, wy, DW_1, DA_1, HANDOVER(12), HANDOVER_N(), HANDOVER_N(), HANDOVER_B());                 \
        HSTEP(S, 1, (S) ^ 1, 0, wy, wx, DW_0, DA_0, HANDOVER_N(), HANDOVER(20), HANDOVER(17), HANDOVER(16));           \
    } while (0)
// Barriers: the four counted hand-overs publish A1(k), W0(k+1), A0(k+1), W1(k+1) before their first reads.  Regions: W1 / A1 of
// stage S ^ 1 were read last in groups 1 / 2 of the half step before this K step and are re-filled from group 1 / 3 on - three
// barriers later; W0 / A0 of stage S are read last in groups 3 / 4 of the first half and re-filled from group 1 / 3 of the
// second: the barrier after group 4 of the first half is theirs.  The other three group ends hand nothing over.

// epilogue of one quarter (A half I, W half J; rows m0 + I * 192 + wr * 96 .., columns n0 + J * 128 + wc * 64 ..): store_tile's
// arithmetic (rbf, gelu_erf_fast, x + rbf(g v)); column tiles nt = 2 q / 2 q + 1 exchanged between lane rows fq = 2 k / 2 k + 1,
// 16-byte stores.  The residual may alias C: every element is loaded and stored by lanes of the same wave, and a wave's loads of
// a quarter all precede its stores of that quarter (a quarter, not a half as in store_tile: beside the 128 accumulator registers
// that live in VGPRs a half's 112 gate / residual registers do not fit).
// Addresses are a uniform tile base + ONE 32-bit lane offset per operand (launcher: 384 rows of C / R span < 2^31 bytes).
template <int EPI, int I, int J>
static __device__ __forceinline__ void store_quarter384(f32x4_t (&acc)[2][6][2][4], bf16_t* C, int64_t N, int64_t ldc,
                                                        const bf16_t* __restrict__ gate, const bf16_t* R, int64_t ldr,
                                                        int64_t rpb, int64_t m0, int64_t n0, int wr, int wc, int fr, int fq) {
    const int row = I * 192 + wr * 96 + fr;                                // + 16 mt
    char* cbase = reinterpret_cast<char*>(C + m0 * ldc + n0);
    const uint32_t coff = (uint32_t)((row * (int)ldc + J * 128 + wc * 64 + (fq & 1) * 16 + (fq >> 1) * 8) * 2);
    uint2 g2[4], r2[6][4];
    if (EPI == DRN_EPI_GATE_RES) {
        const int64_t b = (int64_t)((uint32_t)m0 / (uint32_t)rpb);        // a whole tile lies inside one clip (launcher)
        const char* gbase = reinterpret_cast<const char*>(gate + b * N + n0);
        const char* rbase = reinterpret_cast<const char*>(R + m0 * ldr + n0);
        const uint32_t goff = (uint32_t)((J * 128 + wc * 64 + fq * 4) * 2);
        const uint32_t roff = (uint32_t)((row * (int)ldr) * 2) + goff;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            g2[nt] = *reinterpret_cast<const uint2*>(gbase + (goff + (uint32_t)(nt * 32)));
#pragma unroll
            for (int mt = 0; mt < 6; ++mt)
                r2[mt][nt] = *reinterpret_cast<const uint2*>(rbase + (roff + (uint32_t)(mt * 16 * (int)ldr * 2) + (uint32_t)(nt * 32)));
        }
    }
#pragma unroll
    for (int mt = 0; mt < 6; ++mt)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint2 o[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int nt = 2 * q + h;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = rbf(acc[I][mt][J][nt][r]);
                if (EPI == DRN_EPI_GELU) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = gelu_erf_fast(v[r]);
                } else if (EPI == DRN_EPI_GATE_RES) {
                    const uint2 gg = g2[nt], rr = r2[mt][nt];
                    const float g[4] = {bflo(gg.x), bfhi(gg.x), bflo(gg.y), bfhi(gg.y)};
                    const float x[4] = {bflo(rr.x), bfhi(rr.x), bflo(rr.y), bfhi(rr.y)};
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(g[r] * v[r]);
                }
                o[h].x = pack_bf2(v[0], v[1]);
                o[h].y = pack_bf2(v[2], v[3]);
            }
            const auto sx = __builtin_amdgcn_permlane16_swap(o[0].x, o[1].x, false, false);
            const auto sy = __builtin_amdgcn_permlane16_swap(o[0].y, o[1].y, false, false);
            const u32x4_t val = {sx[0], sy[0], sx[1], sy[1]};
            *reinterpret_cast<u32x4_t*>(cbase + (coff + (uint32_t)(mt * 16 * (int)ldc * 2) + (uint32_t)(q * 64))) = val;
        }
}

template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void gemm384_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W, bf16_t* C, int64_t M, int64_t N, int64_t K,
                    int64_t lda, int64_t ldw, int64_t ldc, const bf16_t* __restrict__ gate, const bf16_t* R, int64_t ldr,
                    int64_t rpb, int GROUP) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];     // G384_LDS, the ONLY LDS object
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int tiles_m = (int)(M / G384_BM), tiles_n = (int)(N / G384_BN);
    const int nk = (int)(K / G384_BK);
    int64_t m0, n0;
    tile_of384(blockIdx.x, tiles_m * tiles_n, tiles_m, tiles_n, GROUP, m0, n0);
    const int dma_off = wave * 1024;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(g384_lptr_t)smem;     // LDS byte address of the object (the DMA's M0)
    const int fr = lane & 15, fq = lane >> 4;
    int offa[2], offw[2];
    {
        const int ra = wr * 96 + fr;                                   // + 16 mt
        const int rw = wc * 64 + fr;                                   // + 16 nt
        offa[0] = ra * 128 + ((fq ^ ((ra >> 1) & 7)) << 4);
        offw[0] = rw * 128 + ((fq ^ ((rw >> 1) & 7)) << 4);
        offa[1] = offa[0] ^ 64;
        offw[1] = offw[0] ^ 64;
    }
    // DMA: piece 4 p + wave = rows 32 p + 8 wave + (lane >> 3) of the half-tile; ((row >> 1) & 7) does not depend on p
    const char* abase = reinterpret_cast<const char*>(A + m0 * lda);
    const char* wbase = reinterpret_cast<const char*>(W + n0 * ldw);
    uint32_t voffa[6], voffw[4];
    {
        const int r = wave * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
#pragma unroll
        for (int p = 0; p < 6; ++p) voffa[p] = (uint32_t)(((r + 32 * p) * (int)lda + c * 8) * 2);
#pragma unroll
        for (int p = 0; p < 4; ++p) voffw[p] = (uint32_t)(((r + 32 * p) * (int)ldw + c * 8) * 2);
    }
    const int64_t a1off = 192 * lda * 2, w1off = 128 * ldw * 2;      // second halves, bytes
    f32x4_t acc[2][6][2][4];         // [i][mt][j][nt]
    bf16x8_t af[6], wx[4], wy[4];    // A fragments [mt]; the two W fragment buffers [nt] (roles swap every half step)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int mt = 0; mt < 6; ++mt)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[i][mt][j][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // ---- prologue: the queue as the loop expects to find it - K step 0 [W0 A0 W1 A1], then W0 / A0 of K step 1 (nk >= 2: launcher)
#pragma unroll
    for (int p = 0; p < 4; ++p) DMA_W(0, p, wbase, 0);
#pragma unroll
    for (int p = 0; p < 6; ++p) DMA_A(0, p, abase, 0);
#pragma unroll
    for (int p = 0; p < 4; ++p) DMA_W(1, p, wbase + w1off, 0);
#pragma unroll
    for (int p = 0; p < 6; ++p) DMA_A(1, p, abase + a1off, 0);
#pragma unroll
    for (int p = 0; p < 4; ++p) DMA_W(0, p, wbase + 2 * G384_BK, 1);
#pragma unroll
    for (int p = 0; p < 6; ++p) DMA_A(0, p, abase + 2 * G384_BK, 1);
    asm volatile("s_waitcnt vmcnt(20)" ::: "memory");                  // W0(0), A0(0): 4 + 6 + 4 + 6 younger pieces
    __builtin_amdgcn_s_barrier();
    FENCE();
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) wx[nt] = LDW(0, 0, nt, 0);
#pragma unroll
    for (int mt = 0; mt < 6; ++mt) af[mt] = LDA(0, 0, mt, 0);
    FENCE();
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");                  // W1(0): read in group 1 of the first half step
    __builtin_amdgcn_s_barrier();
    FENCE();
    // ---- K loop; requests past the end re-request the last K step into regions nobody reads any more: the counts stay uniform
#define DW_1(P) DMA_W(1, P, wbase + w1off + (int64_t)kd1 * (2 * G384_BK), sn)
#define DA_1(P) DMA_A(1, P, abase + a1off + (int64_t)kd1 * (2 * G384_BK), sn)
#define DW_0(P) DMA_W(0, P, wbase + (int64_t)kd2 * (2 * G384_BK), sc)
#define DA_0(P) DMA_A(0, P, abase + (int64_t)kd2 * (2 * G384_BK), sc)
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        {
            const int kd1 = kt + 1, kd2 = min(kt + 2, nk - 1);
            constexpr int sc = 0, sn = 1;
            KSTEP(0, kd1, kd2);
        }
        {
            const int kd1 = min(kt + 2, nk - 1), kd2 = min(kt + 3, nk - 1);
            constexpr int sc = 1, sn = 0;
            KSTEP(1, kd1, kd2);
        }
    }
    if (kt < nk) {
        const int kd1 = nk - 1, kd2 = nk - 1;
        constexpr int sc = 0, sn = 1;
        KSTEP(0, kd1, kd2);
    }
    // the re-requests past the last K step: nothing lands after exit; and the last MFMAs' results are written back before hipcc's
    // own instructions read them (it pads no hazard of an asm statement)
    asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    // every epilogue address derives from these two: defined HERE, so that none of that arithmetic is hoisted above the loop into
    // registers that stay live through it
    int efr = fr, efq = fq;
    asm volatile("" : "+v"(efr), "+v"(efq));
    // (the quarters whose accumulators live in VGPRs first: their registers are free for what follows)
    store_quarter384<EPI, 1, 0>(acc, C, N, ldc, gate, R, ldr, rpb, m0, n0, wr, wc, efr, efq);
    store_quarter384<EPI, 1, 1>(acc, C, N, ldc, gate, R, ldr, rpb, m0, n0, wr, wc, efr, efq);
    store_quarter384<EPI, 0, 0>(acc, C, N, ldc, gate, R, ldr, rpb, m0, n0, wr, wc, efr, efq);
    store_quarter384<EPI, 0, 1>(acc, C, N, ldc, gate, R, ldr, rpb, m0, n0, wr, wc, efr, efq);
}

template <int EPI>
static int launch384(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                     int64_t ldc, const void* gate, const void* residual, int64_t ldr, int64_t rpb, hipStream_t st) {
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm384_kernel<EPI>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, G384_LDS);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const int group = drn_gemm_settings().group;           // tile-rows per L2 band (DRN_GEMM_GROUP: A/B experiments)
    const int64_t tiles = (M / G384_BM) * (N / G384_BN);
    gemm384_kernel<EPI><<<dim3((unsigned)tiles), dim3(256), G384_LDS, st>>>(
        (const bf16_t*)A, (const bf16_t*)W, (bf16_t*)C, M, N, K, lda, ldw, ldc, (const bf16_t*)gate, (const bf16_t*)residual, ldr,
        rpb, group);
    return drn_launch_status();
}

// called from gemm.hip (tile kernel 5); pointer / alignment arguments already validated there.  drn_gemm384_ok (gemm_plan.h) is what
// the kernel needs beyond those checks: the planner asks it before it names this kernel, and nothing is launched without it
static_assert(G384_BM == 384 && G384_BN == 256 && G384_BK == 64, "drn_gemm384_ok (gemm_plan.h) spells the tile out");
int drn_gemm384_dispatch(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                         int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rpb,
                         void* stream, const int64_t* blk) {
    if (lda < K || ldw < K || !drn_gemm384_ok(M, N, K, gemm_ldmax(lda, ldw, ldc, ldr, epilogue), epilogue, rpb, blk)) return DRN_EINVAL;
    if (rpb > M || rpb <= 0) rpb = M;
    hipStream_t st = (hipStream_t)stream;
    switch (epilogue) {
        case DRN_EPI_NONE: return launch384<DRN_EPI_NONE>(A, W, C, M, N, K, lda, ldw, ldc, gate, residual, ldr, rpb, st);
        case DRN_EPI_GELU: return launch384<DRN_EPI_GELU>(A, W, C, M, N, K, lda, ldw, ldc, gate, residual, ldr, rpb, st);
        case DRN_EPI_GATE_RES: return launch384<DRN_EPI_GATE_RES>(A, W, C, M, N, K, lda, ldw, ldc, gate, residual, ldr, rpb, st);
        default: return DRN_EINVAL;
    }
}
