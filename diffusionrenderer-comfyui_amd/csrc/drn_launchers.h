// Internal host-side launchers that one .hip defines and another calls (not part of the C ABI): declared HERE only, included by
// definer and caller alike, so a signature cannot drift between the two.  Arguments are validated by the public entry that calls.
#pragma once
#include "drn_common.h"
#include "gemm_plan.h"

struct ConvGeom;

// ---- attention.hip: the merge of split-KV partials (bf16 and / or MX output; oq != NULL: the MX epilogue); attention_mx.hip's
// split-KV form writes the same partials and ends in this launch too
void drn_attention_combine_launch(const float* opart, const float* mlpart, void* o, int nsplit, int batch, int heads, int64_t Sq,
                                  int64_t ldo, int64_t bso, float scale_log2e, void* oq, void* os, int64_t mx_bs, hipStream_t st);
// ---- attention16.hip: attention_fwd_kernel's twin on v_mfma_f32_16x16x32_bf16 (same grid, same arguments); oq != NULL (unsplit
// launches only): the MX-writing instantiation
void drn_attention16_launch(const void* q, const void* k, const void* v, void* o, int heads, int64_t Sq, int64_t Sk, int64_t ldq,
                            int64_t ldk, int64_t ldv, int64_t ldo, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso,
                            float scale_log2e, int nqb, int64_t total, int nsplit, int64_t kv_chunk, float* opart, float* mlpart,
                            hipStream_t st, void* oq, void* os, int64_t mx_bs);

// ---- gemm.hip: the process's GEMM settings (gemm_plan.h: the A/B switches, read once; .group = DRN_GEMM_GROUP for the tile launchers)
const GemmSettings& drn_gemm_settings();
// ---- gemm.hip: drn_gemm_bf16 with GemmShape::measured384 set (the caller's own A/B stands in for kGemm384Measured)
int drn_gemm_bf16_measured384(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                              int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                              void* stream);
// ---- gemm256s.hip: 256x256x64 tile, streamed schedule (tile kernel 1), and its fp32 K slices
int drn_gemm256s_dispatch(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                          int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rpb,
                          void* stream, const int64_t* blk);
int drn_gemm256s_partial(const void* A, const void* W, float* partial, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                         int splits, void* stream, bool wring_ok);
// ---- gemm384.hip: 384x256x64 tile at one wave per SIMD (tile kernel 5): whole tiles, plain layouts, K >= 128, and for the gated
// residual every tile inside one clip; drn_gemm384_ok (gemm_plan.h) is that test, the dispatch returns DRN_EINVAL without it
int drn_gemm384_dispatch(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                         int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rpb,
                         void* stream, const int64_t* blk);
// ---- gemm144.hip: 144x256x64 kernel (token bands of sequence parallelism: M = 2304 k)
int drn_gemm144_dispatch(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                         int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rpb,
                         void* stream, const int64_t* blk);
// ---- gemm_tall.hip: the few-token kernel.  splits == 1: C = epi(...) directly; splits > 1: fp32 slices into `partial`
int drn_gemm_tall_dispatch(const void* A, const void* W, void* C, float* partial, int64_t M, int64_t N, int64_t K, int64_t lda,
                           int64_t ldw, int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr,
                           int64_t rpb, int splits, void* stream);
// ---- gemm.hip: the reduce launch of a split-K product: sum of the fp32 slices [splits][M][N] + epilogue (bf16 and MXFP8 slices)
int drn_gemm_splitk_reduce(const void* workspace, int splits, void* C, int64_t M, int64_t N, int64_t ldc, int epilogue,
                           const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch, void* stream);
// ---- gemm_mx.hip: the 256 x 256 MXFP8 kernel with the GELU -> MX epilogue (drn_gemm_mxfp8_gelu_mx in gemm_mx_tall.hip validates
// and dispatches)
int drn_gemm_mx_gelu_mx_launch(const void* A, const void* SA, const void* W, const void* SW, void* CQ, void* CS, int64_t M, int64_t N,
                               int64_t K, void* stream);

// ---- conv256s.hip: the streamed 256x256 kernel for the big convolutions
bool drn_conv256s_ok(const ConvGeom& g, int C, int N, int64_t ldc, int64_t ldr, bool has_residual, bool out_f32, const void* y,
                     const void* residual);
int drn_conv256s_launch(const void* x, const void* w, const void* bias, void* y, const void* residual, const ConvGeom& g, int C,
                        int N, int64_t ldw, int64_t ldc, int64_t ldr, void* stream);

// ---- the host prologue the bf16 and the MXFP8 attention launchers share (each keeps its own operand checks in front): the MX
// output contract, the key chunks of a split launch, the grid and the carve of the split-KV workspace into opart | mlpart.
struct AttnLaunch {
    int64_t mx_bs;              // MX output: rows between two clips (bso / ldo); 0 without oq
    int64_t kv_chunk;           // keys per chunk (a multiple of the key tile; Sk when unsplit)
    int nsplit;                 // chunks that hold keys (<= the nsplit asked for: no empty chunk)
    int64_t nqb, total;         // q-blocks of q_rows queries; workgroups = nqb * heads * batch * nsplit
    float* opart;               // [nsplit][batch][Sq][heads][128] fp32, then mlpart [..][heads][2]; NULL when unsplit
    float* mlpart;
    float scale_log2e;
};
// mx_body: whether the selected kernel body can write the MX output at all
static inline int drn_attention_prologue(AttnLaunch* L, void* oq, void* os, bool mx_body, int batch, int heads, int64_t Sq, int64_t Sk,
                                         int64_t ldo, int64_t bso, float scale, int nsplit, void* workspace, int q_rows,
                                         int key_tile) {
    L->mx_bs = 0;
    if (oq) {
        // MX output: rows of heads * 128 elements, contiguous; clip b starts bso / ldo rows after clip b - 1 (the bf16 geometry)
        DRN_CHECK_ARG(os && mx_body && ldo == (int64_t)heads * 128 && bso >= 0 && bso % ldo == 0);
        DRN_CHECK_ARG(((uintptr_t)oq & 7) == 0 && ((uintptr_t)os & 3) == 0);
        L->mx_bs = bso / ldo;
        DRN_CHECK_ARG(batch == 1 || L->mx_bs >= Sq);
    }
    L->kv_chunk = Sk;
    L->nsplit = nsplit;
    if (nsplit > 1 && Sq > 0) {
        DRN_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && batch <= 65535);
        L->kv_chunk = ((Sk + nsplit - 1) / nsplit + key_tile - 1) / key_tile * key_tile;
        L->nsplit = (int)((Sk + L->kv_chunk - 1) / L->kv_chunk);             // no empty chunk
    }
    L->nqb = (Sq + q_rows - 1) / q_rows;
    L->total = L->nqb * heads * batch * L->nsplit;
    DRN_CHECK_ARG(L->total < (1ll << 31));
    L->scale_log2e = scale * 1.44269504088896340736f;
    L->opart = (float*)workspace;
    L->mlpart = L->opart ? L->opart + (int64_t)L->nsplit * batch * Sq * heads * 128 : nullptr;
    return DRN_OK;
}
