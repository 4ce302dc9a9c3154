// Which kernels a bf16 GEMM call launches, on which rows: a pure function of the settings and the call's shape.  Host only, nothing
// of the HIP runtime: gemm.hip executes these plans and reports them (drn_gemm_plan_describe), a plain C++ compiler can sweep them.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "drn.h"

// kernel ids as the ABI reports them: 128^2 (gemm.hip), 256^2 streamed (gemm256s.hip), 144x256 (gemm144.hip), 384x256 (gemm384.hip),
// the few-token kernel (gemm_tall.hip)
enum { GEMM_K128 = 0, GEMM_K256 = 1, GEMM_K144 = 2, GEMM_K384 = 5, GEMM_KTALL = 6 };

// The A/B switches, read once, and drn_gemm_force_tile's value.  DRN_GEMM256=0 / DRN_GEMM144=0 / DRN_GEMM384=0 / DRN_GEMM_TALL=0 /
// DRN_SPLITK256=0 switch a kernel off, DRN_GEMM_TAIL=0 the tail split; DRN_GEMM144=2 and DRN_GEMM384=2 take that tile wherever it
// can run; DRN_GEMM144_COST is the 144-row tile's cost in the model below; DRN_GEMM_GROUP = tile-rows per L2 band of the tile kernels.
struct GemmSettings {
    int mode256 = 1, mode144 = 1, tail = 1, mode384 = 1, tall = 1, splitk256 = 1, group = 4;
    double cost144 = 0.64;
    // drn_gemm_force_tile: -1 automatic; 0 / 1 / 2 / 5 that kernel for every launch (5: a launch it cannot take is refused); 3 = 1;
    // 4 = 1 with the split-K slices of the few-token path on the 2 + 2 stage kernel instead of the weight-ring kernel (tests, A/B)
    int force_raw = -1, force = -1;                        // as given (the queries echo it), and the kernel it stands for
    bool slices_avoid_ring = false;
    void set_force(int tile) {
        force_raw = tile;
        force = tile < 0 ? -1 : (tile == 3 || tile == 4) ? GEMM_K256 : (tile == 1 || tile == 2 || tile == 5) ? tile : GEMM_K128;
        slices_avoid_ring = tile == 4;
    }
};
static inline GemmSettings gemm_settings_from_env() {
    GemmSettings s;
    const auto on = [](const char* name) { const char* e = getenv(name); return (e && e[0] == '0') ? 0 : 1; };
    const auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    s.mode256 = on("DRN_GEMM256"), s.tail = on("DRN_GEMM_TAIL"), s.tall = on("DRN_GEMM_TALL"), s.splitk256 = on("DRN_SPLITK256");
    s.mode144 = num("DRN_GEMM144", 1), s.mode384 = num("DRN_GEMM384", 1), s.group = num("DRN_GEMM_GROUP", 4);
    if (const char* e = getenv("DRN_GEMM144_COST")) s.cost144 = atof(e);
    if (s.mode384 < 0 || s.mode384 > 2) s.mode384 = 1;
    if (s.group < 1) s.group = 4;
    return s;
}

// blk = {a_shift, a_block_stride, c_shift, c_block_stride}; shift 62 = plain layout.  rows_per_batch: rows of one clip.
struct GemmShape {
    int64_t M, N, K, lda, ldw, ldc, ldr;
    int epilogue;
    int64_t rows_per_batch, blk[4];
    // the caller measured the 384 x 256 tile faster on THIS product in its own launch sequence (drn_gemm_bf16_measured384: the
    // DiT forward's block linears, dit_forward.hip) - stands in for an entry on kGemm384Measured, every other rule holds
    bool measured384 = false;
    bool blocked() const { return blk[0] != 62 || blk[2] != 62; }
    // B clips stacked along the rows: tile kernel and tail split decide the accumulation order of an output element, so both are
    // chosen from ONE clip's rows - a clip then gets the same bits whatever it is batched with (the reference steps its G-buffer
    // passes / CFG halves one clip at a time, nodes.py:187-213)
    bool batched() const { return rows_per_batch > 0 && rows_per_batch < M && M % rows_per_batch == 0 && !blocked(); }
    int64_t clip_rows() const { return batched() ? rows_per_batch : M; }
};
// the largest row stride among the operands (the 384-row kernel addresses a tile with 32-bit lane offsets)
static inline int64_t gemm_ldmax(int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int epilogue) {
    int64_t ld = lda > ldw ? lda : ldw;
    if (ldc > ld) ld = ldc;
    return (epilogue == DRN_EPI_GATE_RES && ldr > ld) ? ldr : ld;
}
static inline int gemm_log2_exact(int64_t v) {
    int s = 0;
    while (s < 62 && (1ll << s) < v) ++s;
    return (1ll << s) == v ? s : -1;
}
// blk of a call with A / C in column blocks ("planes", include/drn.h; block_cols = 0: plain) and that call's own argument checks:
// widths powers of two, >= 64 for A and >= 256 for C, that divide K / N and fit in a row
static inline int gemm_block_shift(int64_t cols, int least, int64_t extent, int64_t stride, int64_t ld) {
    const int sh = cols ? gemm_log2_exact(cols) : 62;
    return (!cols || (sh >= least && extent % cols == 0 && stride % 8 == 0 && ld >= cols)) ? sh : -1;
}
static inline int gemm_shape_set_blocks(GemmShape* p, int64_t a_block_cols, int64_t a_block_stride, int64_t c_block_cols,
                                        int64_t c_block_stride) {
    p->blk[0] = gemm_block_shift(a_block_cols, 6, p->K, a_block_stride, p->lda);
    p->blk[1] = a_block_cols ? a_block_stride : 0;
    p->blk[2] = gemm_block_shift(c_block_cols, 8, p->N, c_block_stride, p->ldc);
    p->blk[3] = c_block_cols ? c_block_stride : 0;
    return (p->blk[0] < 0 || p->blk[2] < 0) ? DRN_EINVAL : DRN_OK;
}
// the part of drn_gemm_bf16's argument checks that the shape decides (the pointers are the entry's own)
static inline bool gemm_shape_ok(const GemmShape& p) {
    if (!(p.M >= 0 && p.N > 0 && p.K > 0 && p.K % 64 == 0 && p.N % 128 == 0)) return false;
    // every launch of a plan stays inside its kernel's grid: rows in 31 bits, and so are the tiles of the smallest tile (a plan of
    // several launches must not find this out at its second launch: DRN_EINVAL means that nothing was launched)
    if (!(p.M < (1ll << 31) && ((p.M + 127) / 128) * (p.N / 128) < (1ll << 31))) return false;
    if (!(p.lda % 8 == 0 && p.ldw % 8 == 0 && p.ldc % 8 == 0 && p.ldw >= p.K)) return false;
    if (!((p.blk[0] != 62 || p.lda >= p.K) && (p.blk[2] != 62 || p.ldc >= p.N))) return false;
    return p.epilogue != DRN_EPI_GATE_RES || (p.ldr % 8 == 0 && p.ldr >= p.N && p.rows_per_batch > 0);
}

// What the 384 x 256 kernel needs beyond those checks: whole tiles, plain layouts (blk == NULL: plain), >= 2 K steps, 32-bit lane
// offsets inside a tile (ldmax: gemm_ldmax), and for the gated residual every tile inside one clip.  Its dispatch refuses the rest.
static inline bool drn_gemm384_ok(int64_t M, int64_t N, int64_t K, int64_t ldmax, int epilogue, int64_t rpb, const int64_t* blk) {
    if (blk && (blk[0] != 62 || blk[2] != 62)) return false;
    if (M < 384 || M % 384 != 0 || N % 256 != 0 || K % 64 != 0 || K < 128) return false;
    if (M >= (1ll << 31) || (M / 384) * (N / 256) >= (1ll << 31)) return false;
    if (ldmax < K || ldmax >= (1ll << 31) || (384 * ldmax + 4096) * 2 >= (1ll << 31)) return false;
    return epilogue != DRN_EPI_GATE_RES || ((rpb <= 0 || rpb > M) ? M : rpb) % 384 == 0;
}

// Tile choice by a wave-quantisation model (measured on MI355X).  Time unit = one 256^2 workgroup owning a CU for the whole
// K loop.  128^2 workgroups run two per CU at ~1000 vs ~1300 TF/s: a full round of 512 takes ~0.65 units.  A 144x256
// workgroup does 56 % of the work of a 256^2 one at 0.85-1.0x its rate: DRN_GEMM144_COST = 0.64 units (measured: M = 2304
// -> 0.79 vs 0.97 ms per DiT block; M = 18432 stays on 256^2).  The 384-row tile is not chosen here but in gemm_plan_clip.
static inline int gemm_pick_tile(const GemmSettings& s, int64_t M, int64_t N, double* cost_out = nullptr) {
    if (cost_out) *cost_out = 1e30;
    if (N < 256 || N % 256 != 0) return GEMM_K128;
    if (s.force >= 0) return s.force;
    const int64_t t256 = ((M + 255) / 256) * (N / 256), t128 = ((M + 127) / 128) * (N / 128), t144 = ((M + 143) / 144) * (N / 256);
    const double c128 = 0.65 * (double)((t128 + 511) / 512);
    const double c256 = (s.mode256 == 1 && M >= 256) ? (double)((t256 + 255) / 256) : 1e30;
    // (well below one round of workgroups the model says nothing - measured at M = 1024, N = 4096: 128 workgroups of 144x256
    //  550 TF/s vs 256 of 128^2 655 TF/s - so the 144-row tile needs at least 3/4 of a round)
    const double c144 = (s.mode144 >= 1 && M >= 144 && t144 >= 192) ? s.cost144 * (double)((t144 + 255) / 256) : 1e30;
    if (s.mode144 == 2 && M >= 144) return GEMM_K144;
    const int best = (c144 < c256 && c144 < c128) ? GEMM_K144 : (c256 <= c128 ? GEMM_K256 : GEMM_K128);
    if (cost_out) *cost_out = best == GEMM_K144 ? c144 : (best == GEMM_K256 ? c256 : c128);
    return best;
}
// a tile id as the queries that predate drn_gemm_plan_describe report it: a forced tile as it was given (3 and 4 stay 3 and 4)
static inline int gemm_tile_echo(const GemmSettings& s, int kernel) { return (s.force >= 0 && kernel == s.force) ? s.force_raw : kernel; }

// The 384 x 256 tile at one wave per SIMD (gemm384.hip): fewer operand pieces per FLOP, and 18 432 rows are 48 whole tiles.  A
// workgroup does 1.5 units of work.  Chosen for ONE clip's rows, and only where all of these hold:
//   * its preconditions (drn_gemm384_ok);
//   * the 384-row tiling fills whole rounds of the 256 CUs, or costs fewer round-equivalents than the plan without it;
//   * the shape is on the list of shapes where an interleaved A/B measured it faster than that plan (profiles/gemm384.txt), or
//     the caller says that it measured this product so (GemmShape::measured384) - a shape that ties or loses, or that nobody
//     measured, keeps that plan.  (DRN_GEMM384=2 skips this rule: A/B runs.)
struct Gemm384Shape { int64_t M, N, K; };
static const Gemm384Shape kGemm384Measured[] = {
    {18432, 4096, 16384},                                  // MLP-down at 18 432 tokens: 1.737 -> 1.665 ms
};
static inline bool gemm384_choice(const GemmSettings& s, const GemmShape& p, int64_t M, double cost_without) {
    if (!s.mode384 || s.force >= 0 || p.blocked()) return false;
    if (!drn_gemm384_ok(M, p.N, p.K, gemm_ldmax(p.lda, p.ldw, p.ldc, p.ldr, p.epilogue), DRN_EPI_GATE_RES, M, nullptr)) return false;
    const int64_t t384 = (M / 384) * (p.N / 256);
    const double cost384 = 1.5 * (double)((t384 + 255) / 256);
    if (t384 % 256 != 0 && !(cost384 < cost_without)) return false;
    if (s.mode384 == 2 || p.measured384) return true;
    for (const Gemm384Shape& m : kGemm384Measured)
        if (m.M == M && m.N == p.N && m.K == p.K) return true;
    return false;
}

// How M rows of ONE clip (one gate row) begin: returns the rows of their first launch and its kernel.  Without the 384-row tile that
// is the tile kernel for the rows that fill whole rounds of 256^2 workgroups and - when the last round would be fractional (72 x 16
// tiles = 4.5 rounds cost 5) - the rest left to the launches that follow, planned in turn with the tile that suits them
// (DRN_GEMM_TAIL=0 switches the split off).  A blocked call never leaves a tail to the 128^2 kernel, which has no blocked layouts.
static inline int64_t gemm_plan_clip(const GemmSettings& s, const GemmShape& p, int64_t M, int* kernel) {
    double cost_all = 0.0;
    *kernel = gemm_pick_tile(s, M, p.N, &cost_all);
    int64_t rows = M;
    if (*kernel == GEMM_K256 && s.tail == 1 && s.force < 0) {
        const int64_t tm = (M + 255) / 256, tn = p.N / 256;
        const int64_t rounds = tm * tn / 256, rem = tm * tn % 256;
        const int64_t tm_main = rounds * 256 / tn;
        if (rounds >= 1 && rem != 0 && tm_main >= 1 && tm_main < tm) {
            double cost_tail = 0.0;
            const int tail_tile = gemm_pick_tile(s, M - tm_main * 256, p.N, &cost_tail);
            if (p.blocked() && tail_tile == GEMM_K128) cost_tail = 1e30;
            const double cost_split = (double)((tm_main * tn + 255) / 256) + cost_tail + 0.02;
            if (cost_split < cost_all - 0.05) {
                cost_all = cost_split;
                rows = tm_main * 256;
            }
        }
    }
    if (gemm384_choice(s, p, M, cost_all)) {
        *kernel = GEMM_K384;
        rows = M;
    }
    return rows;
}

// gemm_tall.hip: one clip of 256 tokens - a workgroup owns all 256 rows x 64 columns over the whole K (no slices where N / 64
// workgroups fill the chip: QKV 192, MLP-up 256), or over a K slice (out-proj, MLP-down: 64 tiles x 4).  Returns the slice
// count (1 = unsplit, fused epilogue), 0 = not this kernel.
static inline int gemm_tall_slices(const GemmSettings& s, int64_t M, int64_t N, int64_t K) {
    if (!s.tall || s.force >= 0 || M != 256 || N % 64 != 0 || K % 64 != 0) return 0;
    const int64_t tiles = N / 64;
    if (tiles >= 192) return 1;
    // K slices only while a slice stays short (out-proj: 64 tiles x 4 slices of 16 K steps, 18 + 5 us against 21 + 9 on the
    // 128^2 path); with 64 K steps per slice every workgroup takes in a quarter of the A panel per slice and the 256^2 slices
    // win (MLP-down: 58 + 5 us here against 43 + 9; 128 x 128 tiles, 4 slices of 64 K steps: 59 us against 58 in all)
    for (int n = 2; n <= 8; n *= 2)
        if (tiles * n >= 192 && tiles * n <= 256 && (K / 64) % n == 0 && K / n >= 1024 && K / n <= 2048) return n;
    return 0;
}

struct GemmLaunch { int kernel; int64_t row0, rows, rows_per_batch; };

// The launch of a call that begins at row `row` (0, then row0 + rows of the launch before, until M): DRN_EINVAL when the call is
// refused - a blocked call that needs the 128^2 kernel, a 384-row launch (forced) on rows that kernel cannot take.  Both can only
// happen at row 0: a forced tile covers the call in one launch, and a tail is only split off where its own kernel is not 128^2.
//   * the few-token kernel, unsplit, where its rule takes one clip's rows: one launch for the call;
//   * ragged clips (gated residual, the last clip shorter) and blocked calls with several clips: one launch with the tile of the
//     whole problem, gates by row / rows_per_batch - no tail split and no 384-row tile, whose tiles must lie inside one clip;
//   * else the plan of one clip (gemm_plan_clip, again on the rows each launch leaves): if one launch covers a clip, one launch
//     covers all clips, otherwise every clip gets its own launches, each told that its rows are one clip.
static inline int gemm_plan_next(const GemmSettings& s, const GemmShape& p, int64_t row, GemmLaunch* L) {
    const int64_t Mb = p.clip_rows();
    *L = GemmLaunch{GEMM_KTALL, row, p.M, p.rows_per_batch > 0 ? p.rows_per_batch : p.M};
    if (!p.blocked() && p.M % 256 == 0 && p.lda >= p.K && gemm_tall_slices(s, Mb, p.N, p.K) == 1) return DRN_OK;
    if (!p.batched() && p.epilogue == DRN_EPI_GATE_RES && p.rows_per_batch < p.M) {
        L->kernel = gemm_pick_tile(s, p.M, p.N);
    } else {
        L->rows = L->rows_per_batch = gemm_plan_clip(s, p, Mb - row % Mb, &L->kernel);
        if (L->rows == Mb) L->rows = p.M;
    }
    if (p.blocked() && L->kernel == GEMM_K128) return DRN_EINVAL;
    if (L->kernel == GEMM_K384 && !drn_gemm384_ok(L->rows, p.N, p.K, gemm_ldmax(p.lda, p.ldw, p.ldc, p.ldr, p.epilogue), p.epilogue,
                                                  L->rows_per_batch, p.blk))
        return DRN_EINVAL;
    return DRN_OK;
}

// ---- split-K for few tokens (weight-streaming regime): `splits` workgroups per output tile, fp32 slices, a reduce launch.
// The slices of a product whose 256 x 256 tiles x splits fill at least 3/4 of the CUs with >= 16 K steps each run on the streamed
// kernel (gemm256s.hip; one workgroup per CU, the A slice read once per 256 output columns instead of once per 128): QKV
// (48 tiles x 4), MLP-up (64 x 4), MLP-down (16 x 16).
static inline int gemm_splitk256_slices(const GemmSettings& s, int64_t M, int64_t N, int64_t K) {
    if (!s.splitk256 || (s.force >= 0 && !s.slices_avoid_ring) || M % 256 != 0 || N % 256 != 0 || K % 64 != 0 || M > 1024) return 0;
    const int64_t tiles = (M / 256) * (N / 256);
    int best = 0;
    for (int n = 2; n <= 16; n *= 2)
        if (tiles * n <= 256 && (K / 64) % n == 0 && K / n >= 1024) best = n;
    return (best && tiles * best >= 192) ? best : 0;
}
// How ONE clip's rows are split along K (the split changes the summation order: it must not depend on the batch), and the kernel
// of the slices.  want <= 0: the split that keeps the CUs busy (splits == 1: none) - the few-token kernel's rule, the 256-row
// slices' rule, else 128^2 slices: at most half of the 512 workgroup slots filled by 128^2 tiles, at most 512 workgroups after the
// split and at least 16 K steps left per split.  want > 1: the kernel that computes the slices of a product split `want` ways,
// the one the rule above names if `want` is its count.
struct GemmSplitK { int splits, kernel; };
static inline GemmSplitK gemm_plan_splitk(const GemmSettings& s, int64_t M, int64_t N, int64_t K, int want) {
    const int tall = gemm_tall_slices(s, M, N, K);
    if (want > 1 ? tall == want : tall != 0) return {tall, GEMM_KTALL};
    const int s256 = gemm_splitk256_slices(s, M, N, K);
    if (want > 1 ? s256 == want : s256 != 0) return {s256, GEMM_K256};
    if (want > 1 || gemm_pick_tile(s, M, N) != GEMM_K128) return {want > 1 ? want : 1, GEMM_K128};
    const int64_t tiles = ((M + 127) / 128) * (N / 128);
    int best = 1;
    for (int n = 2; n <= 8; n *= 2)
        if (tiles * n <= 512 && (K / 64) % n == 0 && K / n >= 1024) best = n;
    return {tiles <= 256 ? best : 1, GEMM_K128};
}
