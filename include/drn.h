/* drn.h - C ABI of libdrn.so: the MI355X (gfx950) kernels behind the DiffusionRenderer
 * denoising hot path (CleanGeneralDIT forward + EDM sampler steps + Cosmos CV8x8x8 tokenizer),
 * the forward renderer's per-frame environment-light projection (drn_env_project; with a light per frame drn_env_cubes and
 * drn_env_project_seq), the
 * nodes' clip ingest with a fit to the model's grid (drn_fit_frames), its way back on the
 * uint8 outputs (drn_restore_frames_u8, with the source as a guide drn_restore_guided_u8) and the join of spatial tiles on them
 * (drn_tile_blend_u8).
 *
 * The reference (eggsbenedicto/DiffusionRenderer-ComfyUI) is pure Python/torch and has no FFI;
 * each entry point below names the reference code (file:line under /root/reference) whose
 * arithmetic it replaces.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (e.g. torch tensor.data_ptr());
 *     the library allocates nothing and keeps no pointer after a call returns;
 *   - bf16 tensors are raw 16-bit words, row-major, innermost dimension contiguous;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); kernels are only
 *     enqueued, never synchronised;
 *   - return value: DRN_OK (0), DRN_EINVAL (-1) for a shape/alignment the kernels do not
 *     support (nothing was launched), or a positive hipError_t from the launch;
 *   - not thread-safe per stream; one host thread per process/GPU (ComfyUI runs nodes serially);
 *   - multi-GPU: one process per GPU.  SURVEY.md 8(b) sketched a `drn_comm_init(ncclUniqueId, rank, world)` entry; it was
 *     NOT built: the library has no communication state at all.  The sequence-parallel exchanges (head <-> token all-to-all,
 *     K|V all-gather; parallel.py) are issued by the host through torch.distributed (backend "nccl" = RCCL over xGMI) on the
 *     tensors the kernels below read and write - drn_gemm_bf16_blocked / drn_permute_021 produce and consume the rank-major
 *     slabs of those exchanges directly.  The MXFP8 switches work under that sharding too: drn_gemm_mxfp8_blocked is the slab
 *     GEMM, and the attention output travels home as the e4m3 elements + scales drn_attention_*_mx writes.  Not built: Q / K|V
 *     sent as e4m3, MXFP8 in the sharded tokenizer, the sharded path on drn_dit_forward.
 *   - drn_attention_bf16: the output base and its row / batch strides must allow 16-byte stores (o % 16 == 0, ldo % 8 == 0);
 *     the K / V tile DMA addresses a row as a 32-bit byte offset from its tile's first row: 64 * ldk * 2 and 64 * ldv * 2 < 2^32.
 */
#ifndef DRN_H
#define DRN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRN_OK 0
#define DRN_EINVAL (-1)

#define DRN_ABI_VERSION 1

/* GEMM epilogues */
#define DRN_EPI_NONE 0      /* C = bf16(acc)                                            nn.Linear */
#define DRN_EPI_GELU 1      /* C = bf16(gelu_erf(bf16(acc)))                            CleanGeneralDIT.py:454-457 */
#define DRN_EPI_GATE_RES 2  /* C = bf16(R + bf16(gate * bf16(acc)))                     CleanGeneralDIT.py:517 */

/* GEMV input activation */
#define DRN_ACT_NONE 0
#define DRN_ACT_SILU 1      /* x <- bf16(silu(x)) before the product                     CleanGeneralDIT.py:342,485 */

int drn_abi_version(void);
const char* drn_error_string(int code);

/* ---- token-parallel GEMM: C[M,N] = epi(A[M,K] . W[N,K]^T), bf16 in, fp32 MFMA accumulate, bf16 out.
 * Replaces every nn.Linear of the DiT blocks (CleanGeneralDIT.py:273-276 q/k/v, :254-257 to_out,
 * :445-447 MLP, :386/:417 patch embed, :555/:590 final linear) plus the GELU (:446) and the gated
 * residual (:517) that follow them.
 * Requirements: K % 64 == 0, N % 128 == 0, lda/ldw/ldc/ldr % 8 == 0, 16-byte aligned bases; M < 2^31 and fewer than 2^31 tiles of
 * 128 x 128 (checked before the first launch of a plan, so that DRN_EINVAL keeps meaning that nothing was launched).
 * gate: [batches, N] bf16 (row r uses batch r / rows_per_batch); residual R: [M, ldr] bf16 (may alias C). */
int drn_gemm_bf16(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K,
                  int64_t lda, int64_t ldw, int64_t ldc, int epilogue,
                  const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                  void* stream);

/* ---- the same product with operands stored in column blocks: logical A[m][k] at
 * A + (k / a_block_cols) * a_block_stride + m * lda + k % a_block_cols, logical C[m][n] at
 * C + (n / c_block_cols) * c_block_stride + m * ldc + n % c_block_cols (block_cols 0 = plain; powers of two, >= 64 for A,
 * >= 256 for C).  New on this path (the reference has no multi-GPU code): the sequence-parallel K|V / Q projections write
 * the rank-major send buffer of the head <-> token all-to-all directly and the output projection reads the rank-major
 * receive buffer, instead of a regroup pass either side.  DRN_EINVAL when the shape would take the 128x128 kernel,
 * with ragged clips (DRN_EPI_GATE_RES, rows_per_batch < M) too; nothing is launched then. */
int drn_gemm_bf16_blocked(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K,
                          int64_t lda, int64_t ldw, int64_t ldc, int epilogue,
                          const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                          int64_t a_block_cols, int64_t a_block_stride, int64_t c_block_cols, int64_t c_block_stride,
                          void* stream);

/* ---- the same product for small M (a few hundred tokens: cfg 1, weight-streaming bound): `splits` workgroups share the K
 * range of every output tile so that enough CUs stream the weight matrix; fp32 partials go to `workspace`
 * (drn_gemm_splitk_workspace_bytes), a second kernel sums them and applies the epilogue.  drn_gemm_splitk_choice returns the
 * split count the dispatcher would use for a shape (1 = plain drn_gemm_bf16). */
int drn_gemm_bf16_splitk(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K,
                         int64_t lda, int64_t ldw, int64_t ldc, int epilogue,
                         const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                         int splits, void* workspace, void* stream);
int64_t drn_gemm_splitk_workspace_bytes(int64_t M, int64_t N, int splits);
/* C_f32[M, N] = A . W^T in fp32 as it leaves the accumulators (M, N multiples of 256, K of 64; 256 x 256 streamed kernel): products
 * whose result feeds a softmax - the tokenizer's one-head spatial attention (CleanVAE.py:50-60 -> diffusers' mid-block attention). */
int drn_gemm_bf16_f32out(const void* A, const void* W, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, void* stream);

/* the K slices alone: fp32 partials [splits][M][N] in `workspace`, no sum, no epilogue (the same slices, bit for bit) */
int drn_gemm_bf16_splitk_partials(const void* A, const void* W, int64_t M, int64_t N, int64_t K,
                                  int64_t lda, int64_t ldw, int64_t rows_per_batch, int splits, void* workspace, void* stream);
int drn_gemm_splitk_choice(int64_t M, int64_t N, int64_t K);

/* ---- tuning hooks of drn_gemm_bf16 (no reference counterpart): which tile kernel the wave-quantisation model picks for an
 * [M, N] output (0: 128x128, 1: 256x256, 2: 144x256; N % 256 != 0 always takes 128x128), and a process-wide override for
 * A/B runs and tests (-1 = automatic). */
int drn_gemm_tile_choice(int64_t M, int64_t N);
void drn_gemm_force_tile(int tile);
/* the plan of drn_gemm_bf16 for plain operands, nothing launched: the tile kernel that takes a clip's first launch (0 / 1 / 2 as
 * above, 5: the 384x256 tile at one wave per SIMD - whole tiles only, taken only for shapes where it measured faster;
 * DRN_GEMM384=0 in the environment switches it off) and, in *main_rows (may be NULL), how many of ONE clip's rows that launch covers
 * (fewer than the clip has: a tail launch follows).  rows_per_batch: rows of one clip (<= 0: M).  drn_gemm_force_tile(5) selects
 * the 384x256 kernel for every launch; one it cannot take returns DRN_EINVAL. */
int drn_gemm_plan_choice(int64_t M, int64_t N, int64_t K, int64_t rows_per_batch, int64_t* main_rows);
/* every launch drn_gemm_bf16 / drn_gemm_bf16_blocked (block_cols as there, 0: plain) would make of these arguments, nothing launched:
 * up to `cap` records of four int64 in `out` (may be NULL) - kernel, first row, rows, rows_per_batch passed on - in launch order;
 * returns their number, -1 where the call would return DRN_EINVAL.  Kernels: 0 / 1 / 2 / 5 as above, 6 = the few-token kernel.  It
 * is the planner the GEMM entries run, not a description of it.  splits > 1: the one slice launch of drn_gemm_bf16_splitk, its
 * kernel 6, 1 (256-row slices) or 0 (128x128 slices).  ldr is read with DRN_EPI_GATE_RES only. */
int drn_gemm_plan_describe(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int epilogue,
                           int64_t rows_per_batch, int64_t a_block_cols, int64_t c_block_cols, int splits, int64_t* out, int cap);
/* tuning hook (tests / A-B runs): the gated-residual epilogue of the 256x256 kernel takes its residual tile through LDS, requested
 * under the last two K steps, when the launch allows it (whole tiles inside one clip, an even number >= 4 of K steps, 16-byte
 * residual rows); 0 makes every launch load it after the loop as the other kernels do (same bits), 1 restores the default,
 * -1 only queries.  Returns the previous setting.  (Environment: DRN_GEMM_RES_PREFETCH=0 disables it for the process.) */
int drn_gemm_force_res_prefetch(int on);
/* tuning hook (tests / A-B runs): tile of the few-token kernel (one clip of 256 rows), 0 = 256 rows x 64 columns, 1 = 128 x 128
 * (same bits), -1 = the default (environment DRN_GEMM_TALL_SHAPE, else built in).  Returns the previous setting. */
int drn_gemm_tall_force_shape(int shape);

/* ---- MXFP8 block linears (opt-in precision, HipDiT(precision="mxfp8"); no reference counterpart).
 * Format (OCP MX v1.0): elements OCP e4m3fn (not fnuz); one E8M0 scale byte (e + 127) per 32 consecutive elements along K.
 * For a block with bf16 absolute maximum amax: e = floor(log2(amax)) - 8, e + 1 if amax / 2^e > 448 (significand above 1.75),
 * clamped to [-127, 127]; an all-zero block gets e = -127.  Element = rne_e4m3fn(x / 2^e), never above 448.  Non-finite
 * inputs are outside the contract.
 * Layouts: elements [rows, K] row-major, contiguous (ld = K), one byte each; scales [rows, K / 32] row-major, one byte each
 * (the scale of elements k .. k+31 of row r at r * (K / 32) + k / 32).  Weights [N, K] and activations [M, K] alike. */
/* X [M, K] bf16 with row stride ldx -> Q [M, K] e4m3 + scales [M, K / 32].  K % 32 == 0, ldx % 8 == 0, X 16-byte and Q 8-byte
 * aligned, M * K / 8 <= 2^31 - 256 (the kernel numbers its 8-element chunks in an int, the last workgroup's idle lanes included). */
int drn_mx_quant_bf16(const void* X, int64_t M, int64_t K, int64_t ldx, void* Q, void* scales, void* stream);
/* host-side count of the launches drn_mx_quant_bf16 has enqueued in this process (reset != 0 zeroes it after reading): lets a
 * test state "this forward issued no quantise launch" without a profiler.  A plain counter on the launch path (one host thread
 * per process, as everywhere in this library).  It counts ENQUEUES, not executions: launches a caller replays from a captured
 * graph are not counted, so the statement only holds for eager forwards. */
int64_t drn_mx_quant_calls(int reset);
/* ---- producers that write their result as MXFP8 themselves (the `_mx` entry points below and next to their bf16 twins).
 * The one rule: a fused producer rounds its result to bf16 exactly where its twin rounds and applies the rule above to THAT bf16
 * value, so (Q, scales) == drn_mx_quant_bf16(what the twin writes), bit for bit, and an MXFP8 forward with fused producers equals
 * one with quantise launches.  Outputs are contiguous in the layouts above; the bf16 output pointer of an `_mx` entry may be NULL
 * (not written).  Every `_mx` entry validates on the host and returns DRN_EINVAL before anything is launched. */
/* MLP-up: CQ | CS [M, N] = MX(bf16(gelu_erf(bf16(dequant(A) . dequant(W)^T)))), dispatched by drn_gemm_mxfp8_splitk_choice on one
 * clip's rows (rows_per_batch, or M) like drn_gemm_mxfp8 / drn_gemm_mxfp8_splitk(splits = 1): choice 0 = the 256 x 256 kernel
 * (any M, ragged rows masked on store), 1 = the few-token kernel (either tile shape).  A choice > 1 (sliced K: the GELU then
 * lives in the reduce launch, which has no MX form) returns DRN_EINVAL: callers keep bf16 + drn_mx_quant_bf16 for that shape.
 * N % 256 == 0, K % 128 == 0, A / W 16-byte, scales and CQ 4-byte aligned. */
int drn_gemm_mxfp8_gelu_mx(const void* A, const void* SA, const void* W, const void* SW, void* CQ, void* CS, int64_t M, int64_t N,
                           int64_t K, int64_t rows_per_batch, void* stream);
/* C[M, N] = epi(dequant(A) . dequant(W)^T) on v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate, bf16 out; the epilogues of
 * drn_gemm_bf16 with the same rounding points (gate [batches, N] bf16, row r uses batch r / rows_per_batch; residual [M, ldr]
 * bf16, may alias C).  A / SA, W / SW in the layouts above.  Any M >= 1; N % 256 == 0 and K % 128 == 0 (DRN_EINVAL
 * otherwise); ldc / ldr % 4 == 0, A / W 16-byte, C / R / gate 8-byte, scales 4-byte aligned. */
int drn_gemm_mxfp8(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N, int64_t K,
                   int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                   void* stream);
/* ---- drn_gemm_mxfp8 with operands stored in column blocks ("planes"), as drn_gemm_bf16_blocked defines them: the MXFP8 forms of
 * the sequence-parallel projections write the rank-major send slabs of the head <-> token all-to-all and the output projection
 * reads the rank-major receive slabs - there the e4m3 elements and scales the attention epilogue wrote, as they travelled.
 *   A: logical A[m][k] at A + (k / a_block_cols) * a_block_stride + m * a_block_cols + k % a_block_cols (bytes; a plane's rows are
 *      contiguous), its scale for block k / 32 at the same decomposition of SA divided by 32: SA + (k / a_block_cols) *
 *      (a_block_stride / 32) + m * (a_block_cols / 32) + (k % a_block_cols) / 32.  a_block_cols % 128 == 0 (a K step of 128
 *      bytes and its 4-byte scale piece never straddle a plane), K % a_block_cols == 0, a_block_stride % 128 == 0 and
 *      >= M * a_block_cols.  a_block_cols 0 = plain (then a_block_stride is ignored).
 *   C: logical C[m][n] at C + (n / c_block_cols) * c_block_stride + m * ldc + n % c_block_cols (elements).  c_block_cols a power
 *      of two >= 256 dividing N, ldc >= c_block_cols, c_block_stride % 4 == 0 and >= (M - 1) * ldc + c_block_cols (planes do not
 *      overlap; rows past M are not stored, so nothing lands in the next plane).  c_block_cols 0 = plain (ldc >= N).
 *   W / SW, gate and the residual stay plain.  Product, rounding points, epilogues and every other requirement are those of
 *   drn_gemm_mxfp8: the same kernel (256 x 256 tile, rings, lane maps, swizzle) with the plane addressing as a template flag, so a
 *   blocked product equals the plain one on the same data bit for bit.  It always runs on that kernel - the few-token kernel has
 *   no blocked layouts.  Anything outside the contract: DRN_EINVAL, nothing launched. */
int drn_gemm_mxfp8_blocked(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N, int64_t K,
                           int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                           int64_t a_block_cols, int64_t a_block_stride, int64_t c_block_cols, int64_t c_block_stride,
                           void* stream);
/* ---- the same product for few tokens (one clip of 256 .. 1024 rows; csrc/gemm_mx_tall.hip): a workgroup owns a tile of one
 * clip's rows x a narrow column band (128 x 128 or 256 x 64) over the whole K or over one of `splits` K slices, so that enough
 * CUs stream the weights.  Operands, format and lane maps are those of drn_gemm_mxfp8.
 * drn_gemm_mxfp8_splitk_choice (host-only): 0 = not a few-token shape, call drn_gemm_mxfp8; s >= 1 = the few-token kernel with s
 * K slices (1 = unsplit, fused epilogue).  A pure function of (M, N, K); callers with B clips stacked along the rows pass ONE
 * clip's rows.  Rule: 0 where the 256 x 256 tiles of drn_gemm_mxfp8 cover 3/4 of the 256 CUs; else M N / 16384 column tiles
 * x the largest power-of-two s with tiles x s <= 256 and at least 8 K steps of 128 per slice.
 * drn_gemm_mxfp8_splitk: splits == 1 runs the fused kernel (same rounding points as drn_gemm_mxfp8); splits > 1 writes fp32
 * slices [splits][M][N] to `workspace` (drn_gemm_splitk_workspace_bytes(M, N, splits): the layout of the bf16 slices) and runs
 * the reduce + epilogue launch of drn_gemm_bf16_splitk.  drn_gemm_mxfp8_splitk_partials: the slices alone (bit for bit the
 * same), for drn_splitk_gate_res_ln_modulate.
 * Contract: M % 256 == 0, at most 1024 rows per clip (rows_per_batch, or M), N % 256 == 0, K % 128 == 0, (K / 128) % splits == 0,
 * 1 <= splits <= 64 (partials: >= 2), a 16-byte aligned workspace when splits > 1, alignments as drn_gemm_mxfp8; anything else
 * returns DRN_EINVAL and launches nothing. */
int drn_gemm_mxfp8_splitk_choice(int64_t M, int64_t N, int64_t K);
int drn_gemm_mxfp8_splitk(const void* A, const void* SA, const void* W, const void* SW, void* C, int64_t M, int64_t N, int64_t K,
                          int64_t ldc, int epilogue, const void* gate, const void* residual, int64_t ldr, int64_t rows_per_batch,
                          int splits, void* workspace, void* stream);
int drn_gemm_mxfp8_splitk_partials(const void* A, const void* SA, const void* W, const void* SW, int64_t M, int64_t N, int64_t K,
                                   int64_t rows_per_batch, int splits, void* workspace, void* stream);
/* tuning hook (tests / A-B runs), as drn_gemm_force_tile: 0 = drn_gemm_mxfp8_splitk_choice returns 0 everywhere (every product on
 * drn_gemm_mxfp8), 1 = the default, -1 = query only; returns the previous setting.  Environment DRN_MX_SMALL_M=0 sets the
 * process default. */
int drn_gemm_mxfp8_force_small_m(int on);
/* tuning hook (tests / A-B runs): tile of the few-token MXFP8 kernel, 0 = 256 rows x 64 columns (3 stages), 1 = 128 x 128
 * (4 stages), -1 = the default (environment DRN_MX_TALL_SHAPE, else built in).  Returns the previous setting. */
int drn_gemm_mxfp8_tall_force_shape(int shape);

/* ---- weight-streaming GEMV family (batch-1 vectors: timestep MLP, AdaLN-LoRA, the 1-key cross-attention).
 * For g in [0,groups), b in [0,batch): y[g,b,:] = epi(W[g] . act(x[g,b,:]))   W[g]: [N,K] bf16
 *   y = bf16(acc); if add: y = bf16(y + add[g,b,n]); if mul: y = bf16(mul[g,b,n] * y)
 * Replaces CleanGeneralDIT.py:358-360 (timestep MLP), :483-488/:500-505 (AdaLN-LoRA), :558-562/:572 (final AdaLN),
 * and to_v/to_out of the cross-attention whose single key makes softmax == 1.
 * Strides are in elements; a stride of 0 shares the operand between groups.  K % 8 == 0. */
int drn_gemv_bf16(const void* x, const void* W, void* y, int64_t N, int64_t K,
                  int groups, int batch,
                  int64_t x_gstride, int64_t x_bstride, int64_t w_gstride,
                  int64_t y_gstride, int64_t y_bstride,
                  const void* add, int64_t add_gstride, int64_t add_bstride,
                  const void* mul, int64_t mul_gstride, int64_t mul_bstride,
                  int act, void* stream);

/* ---- LayerNorm(eps, no affine) + AdaLN modulate, one pass: h = bf16(bf16(LN(x) * bf16(1+scale)) + shift)
 * with the reference's rounding points (CleanGeneralDIT.py:7-11, :481, :506; final layer :587).
 * If add_vec != NULL the row is first updated in place, x <- bf16(x + add_vec[batch]) (the broadcast
 * cross-attention residual, :517 with F8), and LN runs on the updated row.
 * x,h: [rows, D] bf16; shift/scale/add_vec: [batches, D] bf16; batch = row / rows_per_batch. D % 8 == 0, D <= 8192; at most
 * 2^33 - 4 rows (2^31 - 1 workgroups of four rows; DRN_EINVAL beyond, nothing launched). */
int drn_ln_modulate(void* x, const void* add_vec, const void* shift, const void* scale, void* h,
                    int64_t rows, int64_t D, int64_t rows_per_batch, float eps, void* stream);
/* the same with h written as MXFP8: hq [rows, D] e4m3 + hs [rows, D / 32] scales (h: bf16 as above, or NULL).  D % 32 == 0 on top
 * of the contract above, hq 8-byte aligned.  drn_ln_force_kernel selects the form as for drn_ln_modulate (same bits). */
int drn_ln_modulate_mx(void* x, const void* add_vec, const void* shift, const void* scale, void* h, void* hq, void* hs,
                       int64_t rows, int64_t D, int64_t rows_per_batch, float eps, void* stream);
/* ---- the sum of split-K partials, the gated residual (CleanGeneralDIT.py:517) and the NEXT sub-block's LayerNorm + modulate
 * (:481, :506) in one pass over [rows, D] (few-token shapes: drn_dit_forward uses it where a linear was split along K):
 *   x <- bf16(x + bf16(gate * bf16(sum_s partials[s]))) [; x <- bf16(x + add_vec)];  h = modulate(LN(x)).
 * Rounds exactly where drn_gemm_bf16_splitk(DRN_EPI_GATE_RES) followed by drn_ln_modulate rounds: the same bits.
 * partials: fp32 [splits][rows][D]; gate / add_vec / shift / scale: [batches, D] bf16.  1024 < D <= 8192. */
int drn_splitk_gate_res_ln_modulate(const void* partials, int splits, void* x, const void* gate, const void* add_vec,
                                    const void* shift, const void* scale, void* h, int64_t rows, int64_t D,
                                    int64_t rows_per_batch, float eps, void* stream);
/* the same with h as MXFP8 (hq, hs as drn_ln_modulate_mx; h may be NULL); D % 32 == 0. */
int drn_splitk_gate_res_ln_modulate_mx(const void* partials, int splits, void* x, const void* gate, const void* add_vec,
                                       const void* shift, const void* scale, void* h, void* hq, void* hs, int64_t rows, int64_t D,
                                       int64_t rows_per_batch, float eps, void* stream);
/* tuning hook (tests / A-B runs; no reference counterpart): the row statistics come from ONE summation tree that a
 * one-wave-per-row and a four-waves-per-row kernel share (same bits); -1 = chosen by row count, 0 / 1 force either. */
void drn_ln_force_kernel(int which);

/* ---- x[rows,D] <- bf16(x + vec[batch,:]) (stand-alone broadcast residual; same arithmetic as above) */
int drn_bcast_add(void* x, const void* vec, int64_t rows, int64_t D, int64_t rows_per_batch, void* stream);

/* ---- y[b][a][:] = x[a][b][:] for x [A, B, C] bf16 (C % 8 == 0): the regroup either side of the head <-> token all-to-all of
 * the sequence-parallel self-attention (token-major [rows, ranks, C] <-> rank-major [ranks, rows, C]); pure data movement.
 * New on this path: the reference has no multi-GPU code. */
int drn_permute_021(const void* x, void* y, int64_t A, int64_t B, int64_t C, void* stream);

/* ---- RMSNorm over the last dim, fp32 internal: y = bf16(x * rsqrt(mean(x^2)+eps) * w)   CleanGeneralDIT.py:14-33
 * D % 8 == 0, D < 2^31, at most 2^33 - 4 rows (2^31 - 1 workgroups of four rows); DRN_EINVAL otherwise, nothing launched. */
int drn_rmsnorm(const void* x, const void* w, void* y, int64_t rows, int64_t D, float eps, void* stream);

/* ---- per-head RMSNorm(q), RMSNorm(k) + 3-D RoPE, in place (CleanGeneralDIT.py:288-295, :45-84).
 * q,k: [tokens, heads, 128] views with row strides ldq / ldk elements (e.g. slices of the fused QKV GEMM output);
 * wq,wk: [128] bf16; cos,sin: [tokens_per_batch, 128] bf16 host-built tables, NULL = no RoPE.
 * rotate_half pairs lane i with i+64.  token t uses table row pos_offset + (t % tokens_per_batch). head_dim must be 128.
 * Either q or k may be NULL (the sequence-parallel path normalises K first so its all-gather can start early). */
int drn_qk_norm_rope(void* q, void* k, const void* wq, const void* wk, const void* cos, const void* sin,
                     int64_t tokens, int heads, int64_t ldq, int64_t ldk, int64_t tokens_per_batch,
                     int64_t pos_offset, float eps, void* stream);

/* ---- non-causal scaled-dot-product attention, head_dim 128, online softmax in fp32, bf16 P for the PV MFMA.
 * Replaces F.scaled_dot_product_attention + the sbhd<->bhsd permutes + the F1 head flatten
 * (CleanGeneralDIT.py:181-203, :299-304).  q,o: [batch, Sq, heads, 128]; k,v: [batch, Sk, heads, 128] given by
 * element strides (token stride ld*, batch stride bs*; head h at offset h*128). */
int drn_attention_bf16(const void* q, const void* k, const void* v, void* o,
                       int batch, int heads, int64_t Sq, int64_t Sk,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                       int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso,
                       float scale, void* stream);

/* tuning hook (tests / A-B runs; no reference counterpart): the kernel body on v_mfma_f32_16x16x32_bf16 (csrc/attention16.hip)
 * instead of 32x32x16; -1 = DRN_ATT16 from the environment / the build default, 0 / 1 forced.  Same arithmetic contract, a
 * different (equally valid) fp32 summation order. */
void drn_attention_force_shape16(int on);

/* ---- same attention with the keys cut into `nsplit` chunks (flash-decoding style): every (q-block, head, chunk) is a
 * workgroup writing an un-normalised fp32 partial into `workspace`, a second kernel merges them.  Arithmetic per chunk is
 * that of drn_attention_bf16; used when (q-blocks x heads) under-fills the 256 CUs, e.g. the 2304-query token bands of
 * 8-way sequence parallelism (288 workgroups -> 2304).  workspace: drn_attention_splitkv_workspace_bytes(...) bytes. */
int drn_attention_splitkv_bf16(const void* q, const void* k, const void* v, void* o,
                               int batch, int heads, int64_t Sq, int64_t Sk,
                               int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                               int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso,
                               float scale, int nsplit, void* workspace, void* stream);
int64_t drn_attention_splitkv_workspace_bytes(int batch, int heads, int64_t Sq, int nsplit);

/* ---- both attentions with the output written as MXFP8: oq [rows, heads * 128] e4m3 + os [rows, heads * 4] scales, contiguous,
 * where row = b * (bso / ldo) + query (so ldo == heads * 128 and bso % ldo == 0 are required even when o is NULL; a launch over a
 * query sub-range of a plan passes o, oq and os advanced by its first row).  o: bf16 as above, or NULL.  oq 8-byte, os 4-byte
 * aligned.  Only the 16x16x32 body has the epilogue (unsplit: in the kernel; split keys: in the combine pass): with the 32x32x16
 * body selected (DRN_ATT16=0 / drn_attention_force_shape16(0)) these return DRN_EINVAL and drn_attention_mx_available() is 0 -
 * callers then keep the bf16 output and drn_mx_quant_bf16 (the same bytes). */
int drn_attention_bf16_mx(const void* q, const void* k, const void* v, void* o, void* oq, void* os,
                          int batch, int heads, int64_t Sq, int64_t Sk,
                          int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                          int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso,
                          float scale, void* stream);
int drn_attention_splitkv_bf16_mx(const void* q, const void* k, const void* v, void* o, void* oq, void* os,
                                  int batch, int heads, int64_t Sq, int64_t Sk,
                                  int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                                  int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso,
                                  float scale, int nsplit, void* workspace, void* stream);
int drn_attention_mx_available(void);

/* ---- MXFP8 self-attention (opt-in, HipDiT(attention_precision="mxfp8"); csrc/attention_mx.hip; no reference counterpart): both
 * products of the attention run on v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands, the online softmax stays fp32.  The one
 * rule of the MX producers holds: a producer rounds to bf16 where its twin rounds and applies the block rule to THAT value.
 * Formats (elements e4m3fn, scales E8M0 bytes, rule as above):
 *   Q, K: elements [rows, heads * 128], scales [rows, heads * 4] - one per 32 consecutive elements of the head dim - contiguous.
 *   V:    stored TRANSPOSED and quantised along the keys: elements VT[b][head][128][Skp], scales VS[b][head][128][Skp / 32], Skp =
 *         Sk rounded up to 128; a block is 32 consecutive keys of one (head, d); keys >= Sk count as zeros (element byte 0), an
 *         all-zero block gets scale byte 0.
 *   P:    rne_e4m3(p 2^PEXP) under the fixed operand scale 2^-PEXP, p = exp2((s - m) scale log2(e)); s = the fp32 accumulator of
 *         dequant(q) . dequant(k); m = the query's reference maximum: kept while a key tile's maximum is within RESCALE_THR (log2
 *         units) of it, else replaced by that tile's maximum, per query (2^THR 2^PEXP <= 448).  The denominator is the sum of the
 *         QUANTISED p, so numerator and denominator see the same rounding.
 *   Output: bf16 `o` and / or MXFP8 `oq` | `os`, exactly as drn_attention_bf16_mx (any one of o, oq may be NULL; os goes with oq).
 * drn_attention_mxfp8_params (host-only): the key tile, RESCALE_THR and PEXP the kernel was built with. */
int drn_attention_mxfp8_params(int* key_tile, float* rescale_thr, int* pexp);
/* Which self-attention sites of a forward with the switch on take these kernels (host-only, a pure function of one clip's tokens
 * like drn_gemm_mxfp8_splitk_choice): 1 from 2048 tokens per clip, else 0 = that site runs the bf16 attention exactly as with the
 * switch off (measured: slower at 256 tokens, equal at 1024, ahead from 2048).  drn_dit_forward and the per-launch host
 * path both ask it.  drn_attention_mxfp8_force (tests / A-B runs): 1 = every site, 0 = the rule (default), anything else only
 * queries; returns the previous setting. */
int drn_attention_mxfp8_choice(int heads, int64_t S);
int drn_attention_mxfp8_force(int on);
/* drn_qk_norm_rope with the result written as MXFP8: qq | qs and kq | ks, contiguous [tokens, heads * 128] / [tokens, heads * 4] -
 * the bytes of drn_mx_quant_bf16 on what drn_qk_norm_rope writes.  Same strided q / k views, pos_offset, tokens_per_batch; q or k
 * may be NULL (then its outputs are not touched).  write_bf16 (0 / 1): whether the in-place bf16 result is written as well.
 * q / k 16-byte, qq / kq 8-byte aligned. */
int drn_qk_norm_rope_mx(void* q, void* k, const void* wq, const void* wk, const void* cos, const void* sin,
                        void* qq, void* qs, void* kq, void* ks,
                        int64_t tokens, int heads, int64_t ldq, int64_t ldk, int64_t tokens_per_batch,
                        int64_t pos_offset, float eps, int write_bf16, void* stream);
/* v: the bf16 view [batch][Sk][heads][128] (token stride ldv, batch stride bsv, head h at offset h * 128: e.g. the v slice of the
 * fused QKV output) -> vt | vs in the V layout above, zero padding up to Skp included.  ldv, bsv % 8 == 0, v / vt 16-byte, vs
 * 4-byte aligned. */
int drn_mx_quant_vt(const void* v, void* vt, void* vs, int batch, int heads, int64_t Sk, int64_t ldv, int64_t bsv, void* stream);
/* non-causal attention, head_dim 128, on the operands above.  Any Sq >= 1, Sk >= 1 (rows past Sq are not stored, keys past Sk are
 * masked).  Clips are stacked along the rows: clip b's queries start at row b * q_bs of qq | qs, its keys at row b * k_bs of
 * kq | ks; vt | vs are those drn_mx_quant_vt writes for (batch, heads, Sk).  A launch over a query sub-range of a plan passes qq,
 * qs, o, oq and os advanced by its first row (as drn_attention_bf16_mx documents).  o [batch, Sq, heads, 128] by ldo / bso.
 * The split-KV form writes the fp32 partials of drn_attention_splitkv_bf16 (workspace: drn_attention_splitkv_workspace_bytes) and
 * ends in the same combine pass, MX epilogue included.  scale > 0; qq / kq / vt / o 16-byte, oq 8-byte, scales 4-byte aligned;
 * ldo, bso % 8 == 0; with oq: ldo == heads * 128 and bso % ldo == 0.  Anything else: DRN_EINVAL, nothing launched. */
int drn_attention_mxfp8(const void* qq, const void* qs, const void* kq, const void* ks, const void* vt, const void* vs,
                        void* o, void* oq, void* os, int batch, int heads, int64_t Sq, int64_t Sk,
                        int64_t q_bs, int64_t k_bs, int64_t ldo, int64_t bso, float scale, void* stream);
int drn_attention_splitkv_mxfp8(const void* qq, const void* qs, const void* kq, const void* ks, const void* vt, const void* vs,
                                void* o, void* oq, void* os, int batch, int heads, int64_t Sq, int64_t Sk,
                                int64_t q_bs, int64_t k_bs, int64_t ldo, int64_t bso, float scale,
                                int nsplit, void* workspace, void* stream);

/* ---- how drn_dit_forward / the host wrapper cover the (q-block, head) grid of ONE clip with whole rounds of the 256 CUs:
 * plan[3 i + {0,1,2}] = (q_begin, q_end, kv_splits) for launch i; returns the number of launches (1 or 2).  The q-blocks that
 * fill whole rounds run unsplit, a fractional last round runs as a second launch with its keys split (split-KV + combine).
 * Host-only (no GPU needed).  No reference counterpart (the reference calls F.scaled_dot_product_attention). */
int drn_attention_plan(int heads, int64_t Sq, int64_t Sk, int64_t* plan);

/* ---- one whole CleanGeneralDIT forward on one GPU, enqueued by ONE call: patch-embed GEMM, n_sub sub-blocks
 * ({FA, CA, MLP} x 28), final LayerNorm + Linear.  Replaces the module loop of CleanGeneralDIT.py:686-706 (x_embedder,
 * `for block in self.blocks.values()`, final_layer) as a SEQUENCER: every launch is one of the kernels above with the arguments
 * the per-launch host path passes (dit_engine.HipDiT._run), so the results are bit-identical to it; ~570 launches cost the host
 * ~2 ms from here instead of 4-7 ms through ctypes.  Patchify before and unpatchify after stay separate calls.
 * Both precisions of the block linears take it (`precision`).
 * B clips of S tokens are stacked along the rows (row = b S + s; attention runs per clip).  All pointers device memory. */
#define DRN_SUB_FA 0     /* self-attention sub-block      CleanGeneralDIT.py:465-517 with block_type "FA" */
#define DRN_SUB_CA 1     /* cross-attention sub-block: one key -> softmax == 1 -> x += bf16(gate * to_out(to_v(ctx))) */
#define DRN_SUB_MLP 2    /* GPT-2 feed-forward sub-block  CleanGeneralDIT.py:442-462 */
typedef struct drn_dit_sub {
    int32_t kind;        /* DRN_SUB_* */
    int32_t site;        /* AdaLN site: row of the shift / scale / gate tables */
    int32_t ca_index;    /* CA: row of `addvec`; else -1 */
    int32_t reserved;
    const void* w_a;     /* FA: fused q|k|v weights [3D, D];  MLP: layer1 [hidden, D] */
    const void* w_b;     /* FA: to_out [D, D];               MLP: layer2 [D, hidden] */
    const void* qn;      /* FA: RMSNorm weight of q [128] */
    const void* kn;      /* FA: RMSNorm weight of k [128] */
    const void* s_a;     /* precision 1: E8M0 scales of w_a (then w_a / w_b are e4m3 elements); else NULL */
    const void* s_b;     /* precision 1: E8M0 scales of w_b */
} drn_dit_sub;
typedef struct drn_dit_forward_args {
    int64_t struct_bytes;                 /* sizeof(drn_dit_forward_args): ABI check */
    int64_t S, B;                         /* tokens per clip, clips */
    int64_t D, hidden;                    /* model width (heads x 128), MLP width */
    int32_t heads, n_sub;
    const drn_dit_sub* subs;              /* HOST array of n_sub entries */
    const void* shift; const void* scale; const void* gate;     /* AdaLN vectors: site s at base + s * site_stride, [B or 1][D] rows */
    int64_t shift_site_stride, scale_site_stride, gate_site_stride;       /* in elements */
    const void* addvec; int64_t addvec_stride;                  /* CA: bf16(gate * c_i) rows, entry i at addvec + i * stride, [B or 1][D] */
    const void* cos; const void* sin;     /* RoPE tables [S, 128] */
    const void* P; int64_t kpad; const void* w_patch;           /* patchified input [B S, kpad], patch-embed weight [D, kpad] */
    const void* final_shift; const void* final_scale; const void* w_final; int64_t n_final;   /* final layer; w_final [n_final, D] */
    void* X; void* H; void* QKV; void* O; void* U; void* Y;     /* activations: [B S, D] x2, [B S, 3D], [B S, D], [B S, hidden], [B S, n_final] */
    void* gemm_ws; int64_t gemm_ws_bytes;                       /* split-K partials (drn_dit_forward_gemm_workspace_bytes) */
    void* attn_ws; int64_t attn_ws_bytes;                       /* split-KV partials (drn_dit_forward_attn_workspace_bytes) */
    void* timer;                          /* drn_timer_create handle or NULL */
    float eps;
    int32_t precision;                    /* 0: bf16 block linears; 1: MXFP8 (subs carry e4m3 weights + scales; patch embed, final
                                           * layer and AdaLN stay bf16; the attention has its own switch, attn_precision) */
    void* AQ; void* AS; int64_t act_bytes;  /* precision 1: the quantised A operand of the next block linear, elements
                                           * [B S, max(D, hidden)] and scales [B S, max(D, hidden) / 32]; act_bytes = the bytes behind
                                           * both together (drn_dit_forward_mx_act_bytes) */
    int32_t mx_fused;                     /* precision 1 only.  0: every block linear quantises its A operand by launch (above).
                                           * 1: the producers write it as MX themselves - see below.  Anything else: DRN_EINVAL */
    int32_t reserved;
    void* UQ; void* US; int64_t u_act_bytes;  /* mx_fused 1: the MX form of U, elements [B S, hidden] and scales [B S, hidden / 32];
                                           * u_act_bytes = the bytes behind both together (drn_dit_forward_mx_u_bytes) */
    int32_t attn_precision;               /* 0: bf16 self-attention (all-zero trailing fields = exactly the launches above);
                                           * 1: MXFP8 self-attention (below), with either precision of the block linears */
    int32_t reserved2;
    void* mx_attn; int64_t mx_attn_bytes; /* attn_precision 1: scratch for QQ | QS | KQ | KS | VT | VS (drn_dit_forward_mx_attn_bytes) */
} drn_dit_forward_args;
/* Every argument and workspace check is made up front, against the sizers below, before anything is enqueued - also those a
 * launcher further down would make only when its turn comes: kpad % 64 == 0, n_final % 128 == 0, hidden % 128 == 0, D <= 8192,
 * B S < 2^31 (B <= 65535 with a FA sub-block), 16-byte bases for P, w_patch, w_final, X, H, QKV, O, U, Y, both workspaces, AQ, UQ and
 * every w_a / w_b (4-byte for AS, US, s_a, s_b).  A launch that fails ends the call with its code; nothing is enqueued behind it.
 * gemm_ws must hold
 * drn_dit_forward_gemm_workspace_bytes (precision 1: the larger of its patch-embed / final-layer share and
 * drn_dit_forward_mx_gemm_workspace_bytes), attn_ws drn_dit_forward_attn_workspace_bytes when a FA sub-block is present - whatever
 * sub-blocks the forward holds.  DRN_EINVAL therefore always means that nothing was launched. */
int drn_dit_forward(const drn_dit_forward_args* args, void* stream);
/* The same forward in parts (the step cache cuts it behind block 0: step_cache.py): the patch embed if `flags` has
 * DRN_DIT_EMBED, then the sub-blocks [sub_lo, sub_hi) of args->subs, then the final layer if `flags` has DRN_DIT_FINAL - each with
 * the launches drn_dit_forward makes for it, on the same buffers; drn_dit_forward IS the part (0, n_sub, EMBED | FINAL).  Between two
 * parts only X carries state, and a part without FINAL leaves X complete: its last gated-residual linear does not defer its
 * split-K sum to a LayerNorm pass that this call will not make (the same bits as deferring: drn_splitk_gate_res_ln_modulate), so
 * parts that tile [0, n_sub) give drn_dit_forward's Y bit for bit.  (sub_lo == sub_hi is allowed: (n_sub, n_sub, FINAL) is the
 * final layer alone.)  DRN_EINVAL (nothing launched): everything drn_dit_forward refuses (the whole argument block is checked,
 * whatever the part), sub_lo > sub_hi, a range outside [0, n_sub], an unknown flag, and a part without FINAL whose last sub-block
 * is a cross-attention (its add would still be pending in the next LayerNorm pass). */
#define DRN_DIT_EMBED 1
#define DRN_DIT_FINAL 2
int drn_dit_forward_range(const drn_dit_forward_args* args, int sub_lo, int sub_hi, int flags, void* stream);
int64_t drn_dit_forward_args_bytes(void);    /* sizeof the two structs as this library was compiled (binding self-check) */
int64_t drn_dit_sub_bytes(void);
int64_t drn_dit_forward_gemm_workspace_bytes(int64_t B, int64_t S, int64_t D, int64_t hidden, int64_t n_final, int64_t kpad);
int64_t drn_dit_forward_attn_workspace_bytes(int64_t B, int heads, int64_t S);
/* host-only sizers for drn_dit_forward with precision 1: the quantised-activation scratch (AQ and AS together), and the fp32
 * slices of the widest sliced block linear under drn_gemm_mxfp8_splitk_choice (the caller allocates the larger of this and the
 * bf16 figure for gemm_ws).  With precision 1 every block linear runs as drn_mx_quant_bf16 into AQ | AS, then drn_gemm_mxfp8
 * (choice 0), the fused few-token kernel (1) or its slices (> 1: a sliced gated-residual linear defers its sum into the next
 * LayerNorm pass exactly as the bf16 one does).  DRN_EINVAL before any launch when AQ / AS are NULL, act_bytes or gemm_ws_bytes
 * are short, a FA / MLP sub-block lacks weights or scales, or D / hidden are not multiples of 256. */
int64_t drn_dit_forward_mx_act_bytes(int64_t B, int64_t S, int64_t D, int64_t hidden);
/* mx_fused == 1 (all-zero trailing fields = exactly the launches described above): no drn_mx_quant_bf16 launch where a producer
 * can write MX itself.  The LayerNorm in front of a FA / MLP sub-block runs as drn_ln_modulate_mx /
 * drn_splitk_gate_res_ln_modulate_mx into AQ | AS viewed as [B S, D] (H is not written; the final-layer LayerNorm and the scratch
 * pass between two CA blocks stay bf16); q|k|v reads AQ | AS; attention writes O as MX into AQ | AS (drn_attention_*_mx; O is not
 * written); out-proj reads it; MLP-up reads AQ | AS and writes U as MX into UQ | US (drn_gemm_mxfp8_gelu_mx; U is not written);
 * MLP-down reads UQ | US.  A site without a fused producer - the 32x32x16 attention body selected, or an MLP-up whose
 * drn_gemm_mxfp8_splitk_choice is > 1 - alone keeps its bf16 output and the quantise launch: the bytes are the same either way.
 * (No site keeps its launch for a timing reason: every fused producer measured faster than producer + quantise launch at 256,
 * 1024 and 18 432 rows per clip, DESIGN 4c.  Were one slower at a shape, the rule would be per site, from ONE clip's rows.)
 * DRN_EINVAL before any launch when mx_fused is neither 0 nor 1, is 1 with precision 0, or UQ / US are NULL or u_act_bytes is
 * below drn_dit_forward_mx_u_bytes (host-only sizer). */
int64_t drn_dit_forward_mx_u_bytes(int64_t B, int64_t S, int64_t hidden);
/* attn_precision == 1: a FA sub-block runs the q|k|v GEMM, drn_qk_norm_rope_mx (write_bf16 0) and drn_mx_quant_vt into `mx_attn`,
 * the plan loop on drn_attention_mxfp8 / drn_attention_splitkv_mxfp8, then out-proj; with mx_fused the output goes to AQ | AS as MX
 * (O is not written), else to O as bf16.  mx_attn holds, in this order and each 256-byte aligned from a 256-byte aligned base: QQ
 * [B S, D], KQ [B S, D], VT [B][heads][128][Sp], QS [B S, D / 32], KS [B S, D / 32], VS [B][heads][128][Sp / 32], Sp = S rounded up
 * to 128 (host-only sizer below).  DRN_EINVAL before any launch when attn_precision is neither 0 nor 1, or is 1 with mx_attn NULL,
 * misaligned or mx_attn_bytes short.
 * drn_dit_forward_mx_attn_layout (host-only) is the one statement of that layout: out[0 .. 5] = the byte offsets of QQ, KQ, VT, QS,
 * KS, VS from the base of mx_attn, out[6] = the total (what drn_dit_forward_mx_attn_bytes returns), out[7] = Sp.  DRN_EINVAL where
 * drn_dit_forward_mx_attn_bytes returns 0: B, S or D not positive, or D % 128 != 0. */
int64_t drn_dit_forward_mx_attn_bytes(int64_t B, int64_t S, int64_t D);
int drn_dit_forward_mx_attn_layout(int64_t B, int64_t S, int64_t D, int64_t out[8]);
int64_t drn_dit_forward_mx_gemm_workspace_bytes(int64_t B, int64_t S, int64_t D, int64_t hidden);

/* ---- per-launch timing inside drn_dit_forward (the roofline leg of bench.py; no reference counterpart): a pool of HIP event
 * pairs; every `sample_every`-th GEMM (kind 0) and attention (kind 1) call of a forward is bracketed on the launch stream.
 * Read after the stream is synchronised.  The one object this library allocates, owned by the caller via create / destroy. */
void* drn_timer_create(int capacity, int sample_every);
void drn_timer_destroy(void* timer);
int drn_timer_count(void* timer);
int drn_timer_seen(void* timer, int kind);
int drn_timer_read(void* timer, int index, int* kind, float* ms, double* flops, double* bytes);

/* ---- patchify + channel concat: out[b*T*H*W + (t,h,w), (c r m n)] gathered from x | cond | ones-mask
 * (CleanGeneralDIT.py:669-675, :409-414).  x: [B,Cx,Tl,Hl,Wl], cond: [B,Cc,Tl,Hl,Wl] bf16; with_mask appends the
 * all-ones channel; columns [C*pt*ps*ps, ldo) are zero-filled (K padding for the GEMM).  Bit-exact index op.  Tl, Hl, Wl >= 1. */
int drn_patchify_concat(const void* x, const void* cond, void* out, int B, int Cx, int Cc, int with_mask,
                        int Tl, int Hl, int Wl, int pt, int ps, int64_t ldo, void* stream);

/* ---- unpatchify: y[(B T)(H W), (ph pw pt C)] -> out[B, C, T*pt, H*ps, W*ps]  (CleanGeneralDIT.py:709-716). Bit-exact. */
int drn_unpatchify(const void* y, int64_t ldy, void* out, int B, int C, int Tp, int Hp, int Wp, int pt, int ps,
                   void* stream);

/* ---- EDM Euler sampler, fp32 math on bf16 latents (model_diffusion_renderer.py:30-82, :232) */
int drn_edm_scale_input(const void* x, void* out, int64_t n, float c_in, void* stream);
int drn_edm_step(const void* model_out, const void* sample, void* out, int64_t n,
                 float c_skip, float c_out, float sigma, float dt, void* stream);
int drn_cfg_combine(const void* cond, const void* uncond, void* out, int64_t n, float guidance, void* stream);

/* ---- pipeline post-process (diffusion_renderer_pipeline.py:299-318): optional normal re-normalisation blend,
 * (1+v).clamp(0,2)/2, permute to (B,T,H,W,C), *255, truncating uint8 cast.  video: [B,3,T,H,W] bf16. Bit-exact.
 * One kernel serves this entry point and the next: this is drn_postprocess_window_u8 with no carry (prev_tail = ramp_w = NULL,
 * O = 0, ramp_at = 0) writing frames [0, T), and takes its 8-pixels-per-lane or one-pixel-per-lane form by the same rule. */
int drn_postprocess_u8(const void* video, void* out_u8, int B, int T, int H, int W, int normalize_normal, void* stream);

/* ---- the post-process for one WINDOW of a long clip (windows.py): frames [write_lo, write_hi) of the decoded window are
 * written, and the O ramp frames [ramp_at, ramp_at + O) are first cross-faded with the previous window's last O decoded frames:
 *   v = bf16(a + w[f - ramp_at] * (b - a)),  a = prev_tail at frame f - ramp_at, b = the window's value, both widened to fp32;
 * subtract, multiply and add are three separately rounded fp32 operations (no FMA).  Every other frame keeps the window's own
 * bf16 value.  v then takes exactly the chain above.  Bit-exact.
 *   video [B,3,Tw,H,W] bf16 (B passes of one window); prev_tail [B,3,O,H,W] bf16 or NULL (no ramp); ramp_w [O] fp32 on the device,
 *   NULL iff prev_tail is NULL; out_u8 [B, write_hi - write_lo, H, W, 3].  All contiguous.
 * H * W % 8 == 0 with 16-byte aligned inputs and an 8-byte aligned output runs 8 pixels per lane (16-byte loads, 24 contiguous
 * bytes out); anything else one pixel per lane.  DRN_EINVAL (nothing launched): a null video / out_u8, only one of prev_tail /
 * ramp_w, O < 0, ramp_at < 0, ramp_at + O > Tw, not (0 <= write_lo < write_hi <= Tw), a ramp with ramp_at < write_lo < ramp_at + O
 * (a ramp is written whole or not at all), a non-positive size. */
int drn_postprocess_window_u8(const void* video, const void* prev_tail, const void* ramp_w, void* out_u8,
                              int B, int Tw, int H, int W, int O, int ramp_at, int write_lo, int write_hi,
                              int normalize_normal, void* stream);

/* ---- windows that agree (windows.py align_affine / apply_affine; extends the window walk of diffusion_renderer_pipeline.py
 * `_walk`, which is the reference's one decode + post-process, :299-318, run per window).  Two windows are independent samples
 * and describe the same frames only over the overlap: the carry a = prev_tail [B,3,O,H,W] and the new window's frames
 * v = video[:, :, ramp_at : ramp_at + O], both bf16.  Per pass b, over all 3*O*H*W values and in fp64: the population moments
 * n, mean_a, mean_v, var_a, var_v, cov; the gain g = sqrt(var_a / var_v) (moment matching, not the regression slope), g = 1 where
 * var_a or var_v < 2^-20 or cov <= 0, clamped to [0.5, 2]; the offset o = mean_a - g * mean_v; any non-finite moment gives (1, 0).
 *   affine [B,2] fp32 = (g, o), each rounded to fp32 once; moments [B,6] fp64 = (n, mean_a, mean_v, var_a, var_v, cov) or NULL.
 * Store-and-sum, no atomics, identical bits run to run: blocks reduce fixed 8192-value chunks of one pass and channel to five fp64
 * partials (sum a, v, a^2, v^2, a v; products exact in fp32) in `workspace`, then one small launch adds them in index order (64
 * contiguous runs, then the runs in order) and evaluates the rules.  Two launches, no host read, no synchronisation.  H * W % 8 == 0 with 16-byte aligned inputs reads 16 bytes
 * per lane; anything else one value per lane.  workspace: at least drn_window_align_workspace_bytes(B, H, W, O) bytes (host
 * arithmetic only; 0 for a non-positive size), 8-byte aligned, not initialised by the caller.
 * DRN_EINVAL (nothing launched): a null video / prev_tail / affine / workspace, O < 1, ramp_at < 0, ramp_at + O > Tw, a short
 * workspace, video / prev_tail off 2 bytes, affine off 4, moments / workspace off 8, a non-positive size, B > 65535. */
int64_t drn_window_align_workspace_bytes(int B, int H, int W, int O);
int drn_window_align_affine(const void* video, const void* prev_tail, void* affine, void* moments, void* workspace,
                            int64_t workspace_bytes, int B, int Tw, int H, int W, int O, int ramp_at, void* stream);

/* ---- drn_postprocess_window_u8 with two more pointers (the same `_walk` lines, and the carry copy `video[:, :, Tw - O:]` behind
 * them).  affine [B,2] fp32 on the device or NULL: every window value the kernel reads becomes bf16(fp32(g * x) + o) with pass
 * b's (g, o) - two separately rounded fp32 operations, no FMA - before the cross-fade, the normal blend and the clamp chain.
 * carry_out [B,3,O,H,W] bf16 or NULL: receives frames [Tw - O, Tw) of the window, aligned and not cross-faded, in the same launch
 * (blocks stride over the written frames, then the carry frames); it must not be prev_tail or video.  affine = NULL skips the
 * arithmetic: out_u8 holds drn_postprocess_window_u8's bytes and carry_out the raw tail.  Bit-exact.
 * The 8-pixels-per-lane form additionally needs carry_out 16-byte aligned.  DRN_EINVAL (nothing launched): every refusal of
 * drn_postprocess_window_u8, affine off 4 bytes, carry_out off 2, carry_out with O < 1, carry_out == prev_tail or video. */
int drn_postprocess_window_align_u8(const void* video, const void* prev_tail, const void* ramp_w, const void* affine,
                                    void* out_u8, void* carry_out, int B, int Tw, int H, int W, int O, int ramp_at,
                                    int write_lo, int write_hi, int normalize_normal, void* stream);

/* ---- environment light of the forward renderer, turning about +Y over the clip (preprocess_envmap.py:440-450 with the unused
 * per-frame hook `y_rot = rotate_y(0.0)` (:340-348, :442) filled in, then hdr_mapping_official :119-140 and the `* 2 - 1` /
 * permute of nodes.py:283-304).  One launch over T*H*W pixels, one thread per output pixel of one frame: the direction
 * vec[h][w] is rotated by frame t's (cos, sin) = rot[t] (q = vec @ rotate_y(theta_t)[:3,:3].T), negated, looked up in the cube
 * map (major-axis face chosen by `ax >= ay && ax >= az`, then `ay >= az`; per-face bilinear fetch with grid_sample's
 * align_corners=False arithmetic and border clamp - the project's own replacement of nvdiffrast's dr.texture, :446), tone
 * mapped (reinhard + clamp + sRGB -> env_ldr; log1p / log1p(log_scale) + sRGB + clamp -> env_log) and stored at the flipped
 * position (H-1-h, W-1-w), scaled to [-1, 1].  All tensors fp32 and contiguous: cube [6,R,R,3], vec [H,W,3] (latlong_vec),
 * rot [T,2], outputs [3,T,H,W].  Accurate powf / log1pf / division, torch's rounding order.  DRN_EINVAL: a null pointer, R, T, H
 * or W < 1, T*H*W >= 2^31, a pointer not 4-byte aligned. */
int drn_env_project(const float* cube, int R, const float* vec, const float* rot, float* env_ldr, float* env_log,
                    int T, int H, int W, float log_scale, void* stream);

/* ---- environment light that changes over the clip: the cube maps of a run of panoramas (preprocess_envmap.py:263-286
 * apply_hdr_preprocessing, then :161-206 latlong_to_cubemap_official, per frame of an env_map batch of which
 * process_comfyui_tensor :247-261 keeps frame 0 only).  One launch over n*6*R*R cube texels, one thread per texel of one panorama
 * (12 contiguous bytes out).  The sampling grid does not depend on the frame: the host computes it once with the torch
 * expressions of :161-206 (preprocess_envmap.cube_sample_grid), so the kernel evaluates no transcendental.  Per texel and
 * channel, grid_sample(mode="bilinear", padding_mode="border", align_corners=False) in drn_env_project's arithmetic and order
 * (unnormalise and clamp each axis with its own size - the product and the `- 1` in ONE fused multiply-add, as torch's grid_sample
 * builds contract them, where drn_env_project's cube lookup rounds twice - weights `(x0 + 1) - ix` .., nw + ne + sw + se, an
 * out-of-range neighbour contributes 0 * w, no contraction anywhere else).  The clean-up of :263-286 is elementwise and is applied to every tap as it is read:
 * `* brightness` only when brightness != 1.0, nan -> 0, +inf -> 65504, -inf -> 0, clamp to [0, 65504].  Flip and roll are index
 * arithmetic on the source column, the flip before the roll: column c of the cleaned panorama is raw column
 * j = (c - roll) mod We, or We - 1 - j with flip; roll = int(We * env_rot / 360) mod We comes from the host.
 *   latlong [N,He,We,3] raw; grid [6,R,R,2] = (x, y) in [-1, 1]; cubes [n,6,R,R,3] = the cube maps of panoramas n0 .. n0+n-1.
 *   All fp32 and contiguous.
 * DRN_EINVAL (nothing launched): a null pointer, N, He, We or R < 1, n0 < 0, n < 1, n0 + n > N, roll outside [0, We), a pointer
 * not 4-byte aligned, N*He*We*3 or n*6*R*R*3 >= 2^31. */
int drn_env_cubes(const float* latlong, const float* grid, float* cubes, int N, int He, int We, int R, int n0, int n,
                  float brightness, int flip, int roll, void* stream);

/* ---- drn_env_project with a cube map per frame (the same lines, :440-450 / :119-140; the same kernel): frame t looks up cube map
 * cube_of[t] of cubes [n_cubes,6,R,R,3] under rot[t], and is stored at frame t0 + t of outputs [3,T_all,H,W], of which no other
 * frame is touched - so a clip is projected in chunks of frames whose cube maps are built chunk by chunk.  cube_of int32 [T] and
 * rot [T,2] on the device.  cube_of is clamped into [0, n_cubes) before use; what it should hold is checked on the host
 * (native.env_project_seq).  With every cube_of[t] = 0, t0 = 0 and T_all = T this is drn_env_project, bit for bit.
 * DRN_EINVAL (nothing launched): what drn_env_project refuses, a null cube_of, n_cubes < 1, t0 < 0, t0 + T > T_all,
 * T_all*H*W >= 2^31, cube_of not 4-byte aligned. */
int drn_env_project_seq(const float* cubes, int n_cubes, const int32_t* cube_of, int R, const float* vec, const float* rot,
                        float* env_ldr, float* env_log, int T, int t0, int T_all, int H, int W, float log_scale, void* stream);

/* ---- clip ingest with a fit to the model's grid (the nodes' `image.permute(0, 4, 1, 2, 3) * 2.0 - 1.0`, nodes.py:156-190, with
 * a resize, a crop and a time padding in front that the reference does not have; plan and torch specification: fit.py).
 * ONE launch: dst[b][ch][t][y][x] = bf16(2 * acc - 1),
 *   acc = sum_ky y_w[y][ky] * (sum_kx x_w[x][kx] * src[b][t_idx[t]][y_lo + ky][x_lo + kx][ch]),
 * all in fp32 (fma accumulation from 0 in tap order, the row pass first), 2 * acc - 1 rounded once, then round to nearest even.
 *   src [B,Ts,Hs,Ws,3] fp32 and dst [B,3,Td,Hd,Wd] bf16, contiguous; tables on the device: t_idx int32 [Td] (source frame of
 *   every output frame), per axis lo_n int32 [n_out][2] (first source sample, tap count n in 1..K) and w fp32 [n_out][K]
 *   (zero-padded past n; the crop offset is folded into lo).
 * The loops run over every row's own n: a source index outside [lo, lo + n) is never touched and padded weights are not taps, so
 * a single tap of weight 1.0 on both axes copies (bit for bit what `* 2 - 1` and the bf16 cast give).  lo, n and t_idx are
 * clamped into the source before use; what they should hold is checked on the host (native.fit_frames).
 * DRN_EINVAL (nothing launched): a null pointer, a non-positive size, Ky or Kx outside 1..32, Hd or Wd not a multiple of 16,
 * B*3*Td*Hd*Wd or B*Ts*Hs*Ws*3 >= 2^31, src or a table not 4-byte aligned, dst not 16-byte aligned. */
int drn_fit_frames(const float* src, void* dst_bf16, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                   const int* t_idx, const int* y_lo_n, const float* y_w, int Ky,
                   const int* x_lo_n, const float* x_w, int Kx, void* stream);

/* ---- the same ingest from 8-bit frames (what decoded video is, and what the post-process leaves on the device: the uint8
 * G-buffers of the inverse renderer become the forward renderer's conditions without a host round trip; no reference line).
 * ONE launch: drn_fit_frames on the frames unit[src], bit for bit at every geometry, where
 *   unit[i] = fp32(i) / 255.0f, correctly rounded (the division, NOT a multiplication by 1.0f / 255: that differs at 126 of the
 *   256 byte values), which is what `u8.float() / 255.0` gives on the host.
 * From there the arithmetic is drn_fit_frames': fma accumulation from 0 in tap order, the row pass first, 2 * acc - 1 rounded
 * once, round to nearest even.  A single tap of weight 1.0 on both axes gives the bits of
 * `((u8.float() / 255).permute(0, 4, 1, 2, 3) * 2 - 1).to(bf16)`.
 *   src [B,Ts,Hs,Ws,3] uint8, contiguous, at ANY byte alignment; dst [B,3,Td,Hd,Wd] bf16, contiguous; the tables as for
 *   drn_fit_frames, with the same clamping of lo, n and t_idx (what they should hold is checked on the host,
 *   native.fit_frames_u8).  Nothing outside src is read: a row's bytes are fetched with aligned 4-byte loads inside the span the
 *   tile's taps cover, its ragged ends bytewise.
 * DRN_EINVAL (nothing launched): a null pointer, a non-positive size, Ky or Kx outside 1..32, Hd or Wd not a multiple of 16,
 * B*3*Td*Hd*Wd or B*Ts*Hs*Ws*3 (bytes) >= 2^31, a table not 4-byte aligned, dst not 16-byte aligned. */
int drn_fit_frames_u8(const uint8_t* src, void* dst_bf16, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                      const int* t_idx, const int* y_lo_n, const float* y_w, int Ky,
                      const int* x_lo_n, const float* x_w, int Kx, void* stream);

/* ---- the fit's way back: the uint8 result of the post-process resampled to the source's size (no reference line: the reference
 * has neither a fit nor its inverse; this is the inverse of drn_fit_frames for fits that kept the whole picture, and replaces a
 * resize of fp32 frames on the host; plan and torch specification: fit.py, plan_restore / restore_frames).
 * ONE launch: dst[b][t][y][x][ch] = uint8(clamp(rint(acc), 0, 255)),
 *   acc = sum_ky y_w[y][ky] * (sum_kx x_w[x][kx] * src[b][t][y_lo + ky][x_lo + kx][ch]),
 * all in fp32 on the 0..255 scale (fma accumulation from 0 in tap order, the row pass first), rint = round to nearest even.
 *   src [B,Ts,Hs,Ws,3] and dst [B,Td,Hd,Wd,3] uint8, contiguous, at ANY byte alignment; Td <= Ts: frame t of dst comes from frame
 *   t of src (the time padding is cut); any Hd, Wd >= 1.  Tables on the device as for drn_fit_frames: per axis lo_n int32
 *   [n_out][2] and w fp32 [n_out][K], zero-padded past n.
 * lo and n are clamped into the source before use; what they should hold is checked on the host (native.restore_frames).  A
 * single tap of weight 1.0 on both axes copies.  Nothing outside dst is written, nothing outside src is read.
 * DRN_EINVAL (nothing launched): a null pointer, a non-positive size, Td > Ts, Ky or Kx outside 1..32, B*Td*Hd*Wd*3 or
 * B*Ts*Hs*Ws*3 >= 2^31, a table not 4-byte aligned. */
int drn_restore_frames_u8(const uint8_t* src, uint8_t* dst, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                          const int* y_lo_n, const float* y_w, int Ky, const int* x_lo_n, const float* x_w, int Kx, void* stream);

/* ---- the guided way back: the uint8 result of the post-process brought to the source's size with the source picture as a guide
 * (no reference line: the reference has no fit; joint bilateral upsampling, Kopf et al. 2007; plan and torch specification:
 * fit.py, plan_restore_guided / restore_frames_guided).
 * ONE launch.  For output pixel (b, t, y, x), G = guide_hi[bg][t0 + t][y][x][:], q over the taps (y_lo + ky, x_lo + kx), ky
 * outer and kx inner, g(q) = guide_lo[bg][t0 + t][q][:], bg = 0 where Bg == 1 and b otherwise:
 *   r(q) = range_tab[|G_0 - g(q)_0|] * range_tab[|G_1 - g(q)_1|] * range_tab[|G_2 - g(q)_2|] + eps
 *   w(q) = (y_w[y][ky] * x_w[x][kx]) * r(q)
 *   dst[b][t][y][x][ch] = uint8(clamp(rint((sum_q w(q) * src[b][t][q][ch]) / (sum_q w(q))), 0, 255)),
 * all in fp32 on the 0..255 scale (fma accumulation from 0 in tap order, one division), rint = round to nearest even.
 *   src [B,Ts,Hs,Ws,3], guide_lo [Bg,Tg,Hs,Ws,3], guide_hi [Bg,Tg,Hd,Wd,3] and dst [B,Td,Hd,Wd,3] uint8, contiguous, at ANY
 *   byte alignment; Bg is 1 (one guide for every clip) or B; Td <= Ts, 0 <= t0, t0 + Td <= Tg.  Tables on the device as for
 *   drn_restore_frames_u8: per axis lo_n int32 [n_out][2] and w fp32 [n_out][K], zero-padded past n; range_tab fp32 [256] (the
 *   plan's exp(-d^2 / (2 sigma^2)): no transcendental is evaluated on the device).
 * lo and n are clamped into the source before use; what they should hold is checked on the host (native.restore_guided).
 * Nothing outside dst is written, nothing outside src, guide_lo and guide_hi is read.
 * DRN_EINVAL (nothing launched): a null pointer, a non-positive size, Bg not 1 or B, Td > Ts, t0 < 0, t0 + Td > Tg, Ky or Kx
 * outside 1..8, any of the four tensors >= 2^31 bytes, a table not 4-byte aligned, eps <= 0. */
int drn_restore_guided_u8(const uint8_t* src, const uint8_t* guide_lo, const uint8_t* guide_hi, uint8_t* dst,
                          int B, int Bg, int Ts, int Hs, int Ws, int Tg, int t0, int Td, int Hd, int Wd,
                          const int* y_lo_n, const float* y_w, int Ky, const int* x_lo_n, const float* x_w, int Kx,
                          const float* range_tab, float eps, void* stream);

/* ---- spatial tiles: one rendered tile cross-faded into the picture's canvas, in place (no reference line: the reference renders
 * a picture as one sequence; plan and torch specification: tiles.py, plan_tiles / blend_tile).
 * ONE launch.  canvas [frames,H,W,3] and tile [frames,h,w,3] uint8, contiguous, at ANY byte alignment.  For tile-local
 * y in [ry, h), x in [rx, w) and every channel, with a = canvas[f][y_at + y][x_at + x][ch], b = tile[f][y][x][ch] as fp32:
 *   wgt = Wy(y - ry) * Wx(x - rx)       (one fp32 multiply; Wy(i) = wy[i] for i < Oy and 1.0f behind, Wx likewise)
 *   wgt == 1:  canvas <- b               (the canvas is not read)
 *   else:      canvas <- uint8(clamp(rint(a + wgt * (b - a)), 0, 255))
 * subtract, multiply and add three separately rounded fp32 operations (never an FMA), rint = round to nearest even.
 *   wy fp32 [Oy], wx fp32 [Ox] on the device (windows.ramp_weights); NULL exactly where the count is 0.
 * Rows in front of ry and columns in front of rx of the tile are not used.  Nothing outside the rectangle
 * [y_at + ry, y_at + h) x [x_at + rx, x_at + w) of the canvas is written, and nothing outside it is read from the canvas.  Frame
 * bases are 64-bit: the canvas may pass 2^31 bytes, one frame of either side may not.
 * DRN_EINVAL (nothing launched): a null canvas or tile, a size < 1, y_at < 0, x_at < 0, y_at + h > H, x_at + w > W, ry outside
 * [0, h), rx outside [0, w), Oy < 0, Ox < 0, ry + Oy > h, rx + Ox > w, wy == NULL not equivalent to Oy == 0 (wx and Ox likewise),
 * a weight table not 4-byte aligned, a frame of either side of 2^31 bytes or more, more than 2^31 workgroups (frames x 16-row x
 * 128-pixel blocks of the written rectangle). */
int drn_tile_blend_u8(void* canvas, const void* tile, const void* wy, const void* wx, int64_t frames, int H, int W, int h, int w,
                      int y_at, int x_at, int ry, int rx, int Oy, int Ox, void* stream);

/* ---- spatial tiles joined in LATENT space (no reference line for the tiling: the reference samples a picture as one sequence;
 * the arithmetic is the reference sampler's, model_diffusion_renderer.py:30-44 (scale_model_input), :232 (CFG) and :46-82 (step);
 * plan and torch specification: tiles.py, latent_tile / latent_gather / latent_step_join).  A plane is one
 * (pass, channel, latent frame); canvas bf16 [planes,Hc,Wc] and tile bf16 [planes,h,w], contiguous, at ANY 2-byte alignment;
 * x_at, rx, Wc and w may be odd.  Plane bases are 64-bit: a canvas may pass 2^31 elements, one plane of either side may not.
 *
 * drn_latent_tile_gather - the tile's crop of the canvas as the DiT's input, ONE launch instead of slice + contiguous +
 * drn_edm_scale_input (+ torch.cat of the result with itself under CFG):
 *   out[k][plane][r][c] = bf16(fp32(canvas[plane][y_at + r][x_at + c]) * c_in)      for k < copies, copies 1 or 2
 * bit for bit edm_scale_input(crop.contiguous()).  Nothing outside `out` is written; the canvas is read at the crop only.
 * DRN_EINVAL (nothing launched): a null or odd pointer, a size < 1, y_at < 0, x_at < 0, y_at + h > Hc, x_at + w > Wc, copies
 * outside 1..2, a plane of either side of 2^31 elements or more, more than 2^31 workgroups.
 *
 * drn_latent_tile_step_join - CFG combine, Euler step and cross-fade of one tile's DiT output into the NEXT canvas, ONE launch
 * instead of drn_cfg_combine + drn_edm_step on contiguous crops + a torch blend on slices.  For tile-local y in [ry, h),
 * x in [rx, w), with c = model_out, u = uncond, sm = canvas_cur and a = canvas_next at that element, as fp32:
 *   m   = uncond ? bf16(c + bf16(guidance * bf16(c - u))) : c                        (drn_cfg_combine; uncond == NULL: no CFG)
 *   b   = bf16(sm + ((sm - (c_skip * sm + c_out * m)) / sigma) * dt)                 (drn_edm_step, rounding for rounding)
 *   wgt = Wy(y - ry) * Wx(x - rx)       (one fp32 multiply; Wy(i) = wy[i] for i < Oy and 1.0f behind, Wx likewise)
 *   wgt == 1:  canvas_next <- b          (canvas_next is not read)
 *   else:      canvas_next <- bf16(a + wgt * (b - a))
 * subtract, multiply and add three separately rounded fp32 operations (never an FMA), rounded to nearest even into bf16:
 * drn_tile_blend_u8's rule on bf16.  wy fp32 [Oy], wx fp32 [Ox] on the device (windows.ramp_weights); NULL exactly where the
 * count is 0.  Rows in front of ry and columns in front of rx of the tile are not used.  canvas_cur is only read, and only at
 * the tile's rectangle; nothing outside [y_at + ry, y_at + h) x [x_at + rx, x_at + w) of canvas_next is written or read.
 * DRN_EINVAL (nothing launched): a null model_out or canvas, an odd pointer, canvas_cur == canvas_next, a size < 1, a tile
 * outside the canvas, ry outside [0, h), rx outside [0, w), Oy < 0, Ox < 0, ry + Oy > h, rx + Ox > w, wy == NULL not equivalent
 * to Oy == 0 (wx and Ox likewise), a weight table not 4-byte aligned, sigma == 0, a plane of either side of 2^31 elements or
 * more, more than 2^31 workgroups (planes x 16-row x 128-element blocks of the written rectangle). */
int drn_latent_tile_gather(const void* canvas, void* out, int64_t planes, int Hc, int Wc, int h, int w, int y_at, int x_at,
                           float c_in, int copies, void* stream);
int drn_latent_tile_step_join(const void* model_out, const void* uncond, float guidance, const void* canvas_cur,
                              void* canvas_next, const float* wy, const float* wx, int64_t planes, int Hc, int Wc, int h, int w,
                              int y_at, int x_at, int ry, int rx, int Oy, int Ox, float c_skip, float c_out, float sigma, float dt,
                              void* stream);

/* ---- DPM-Solver++(2M) sampler step (no reference line for the solver: the reference samples with first-order EDM Euler; it
 * stands beside model_diffusion_renderer.py:30-82 (scale_model_input, step: the preconditioning c_in / c_skip / c_out is theirs)
 * and :224-234 (the loop and its CFG combine); plan and torch specification: sampler.py, plan_steps / step_reference;
 * DESIGN.md 4l).  ONE launch per step; under CFG it stands for drn_cfg_combine + drn_edm_step + the NEXT step's
 * drn_edm_scale_input + torch.cat([xs, xs]).  Per element i < n, with c = cond, u = uncond, x and h = hist_in as fp32, every
 * fp32 operation rounded on its own (never an FMA):
 *   m        = uncond ? bf16(c + bf16(guidance * bf16(c - u))) : c                  (drn_cfg_combine; uncond == NULL: no CFG)
 *   D        = c_skip * x + c_out * m                                               (drn_edm_step's `denoised`)
 *   s        = b1 * D;  hist_in ? s = s + b0 * h                                    (hist_in == NULL: the history is not read)
 *   x_out    = bf16(a * x + s)
 *   hist_out = D                                                                    (fp32)
 *   scaled_out[k * n + i] = bf16(fp32(x_out) * c_in_next)   for k < copies          (scaled_out == NULL, the last step: not written)
 * cond, uncond, x, x_out: bf16 [n]; hist_in, hist_out: fp32 [n]; scaled_out: bf16 [copies * n], the batch the DiT takes next
 * (copies = 2 under CFG: both halves are the same values).  hist_out may be hist_in; no other two tensors may overlap.  The
 * coefficients (a, b1, b0) come from sampler.plan_steps: (sigma_next / sigma, e, 0) on the first step, (sigma_next / sigma,
 * e (1 + 1 / 2r), -e / 2r) on a middle one, (0, 1, 0) on the step to sigma = 0, with e = 1 - sigma_next / sigma and
 * r = log(sigma_prev / sigma) / log(sigma / sigma_next).  Any alignment on the element's grid; 8 elements per lane where every
 * base pointer (scaled_out + n for the second copy included) is 16-byte aligned, one per lane otherwise: the same bits.
 * DRN_EINVAL (nothing launched): a null cond, x, hist_out or x_out; copies outside 1..2 with scaled_out set; n < 0;
 * hist_in == NULL with b0 != 0; a bf16 pointer off the 2-byte grid or a history pointer off the 4-byte grid.  n == 0: DRN_OK,
 * nothing launched. */
int drn_sampler_step_2m(const void* cond, const void* uncond, float guidance, const void* x, const float* hist_in,
                        float* hist_out, void* x_out, void* scaled_out, int copies, int64_t n, float c_skip, float c_out,
                        float a, float b1, float b0, float c_in_next, void* stream);

/* ---- seed ensembles: N uint8 results of one shape, rendered under N seeds, reduced per pixel (no reference line: the reference
 * renders one sample; the torch specification: ensemble.py, reduce_members).  ONE launch.  members: a HOST array
 * of N device pointers, uint8 [n_bytes] each (they travel to the kernel by value: no device table, no copy); dst: uint8
 * [n_bytes]; spread: uint8 [n_bytes] or NULL (then neither computed nor written).  m_k = member k's byte.
 *   mode 0, median, per byte, in integers: s = the N bytes sorted ascending, lo = s[(N-1)/2], hi = s[N/2], t = lo + hi,
 *     r = t >> 1, and r += r & 1 where t is odd (the two middle values averaged, half to even; odd N: the middle value).
 *     spread = the same rule on d_k = |m_k - r| (the median absolute deviation).
 *   mode 1, mean, per byte, in integers: S = sum m_k, q = S / N, rem = S % N, r = q + 1 where 2 rem > N or (2 rem == N and q is
 *     odd), else q.  spread = the same rule on d_k = |m_k - r|.
 *   mode 2, normal, per pixel of three bytes (n_bytes % 3 == 0), in fp32, every operation rounded on its own (never an FMA):
 *     v_k,c = unit(m_k,c) * 2 - 1, unit(i) = fp32(i) / 255.0f correctly rounded (fit.u8_unit); s_c = v_0,c, then s_c = s_c + v_k,c
 *     for k = 1..N-1 in member order; l2 = (s_x s_x + s_y s_y) + s_z s_z, l = sqrt(l2), d = max(l, 1e-6f), n_c = s_c / d, sqrt and
 *     / correctly rounded; dst = uint8(rint(clamp((n_c + 1) * 127.5f, 0, 255))), rint half to even (a zero sum: 128, 128, 128);
 *     spread = uint8(rint(255 * clamp(1 - l / fp32(N), 0, 1))), one minus the mean resultant length, in all three channels.
 * N = 1: modes 0 and 1 copy (spread 0); mode 2 still renormalises.  Every pointer at any byte alignment: 16 bytes (mode 2: 48
 * bytes, 16 whole pixels) per lane where every base is 16-byte aligned, one byte (one pixel) per lane otherwise - the same bits;
 * 64-bit offsets.  dst and spread may overlap nothing else.
 * DRN_EINVAL (nothing launched): a null members, member or dst; N outside 1..16; mode outside 0..2; n_bytes < 0;
 * n_bytes % 3 != 0 in mode 2; dst == spread; dst or spread equal to a member.  n_bytes == 0: DRN_OK, nothing launched. */
int drn_ensemble_reduce_u8(const void* const* members, int N, void* dst, void* spread, int64_t n_bytes, int mode, void* stream);

/* ---- ensembles that agree: one gain and offset per member and clip, solved on the device in front of the reduce (no reference
 * line; the rule and the torch / numpy specification: ensemble.py, align_solve_members / align_members).  The
 * members are B clips of clip_bytes bytes each (all of T x H x W x 3); member 0 is the space the result lives in.
 *
 * drn_ensemble_align_affine: members: a HOST array of N device pointers, uint8 [B * clip_bytes] each (by value, as in the
 * reduce); affine: fp32 [N][B][2] = (g, o); stats: fp64 [B][N + N * N] = the means, then C row by row, or NULL; workspace: at
 * least drn_ensemble_align_workspace_bytes(N, B, clip_bytes) bytes, not initialised by the caller.  Per clip, with n = clip_bytes:
 *   S_k = sum m_k, S_jk = sum m_j m_k (j <= k), exact integers; mean_k = f64(S_k) / n; C_jk = f64(S_jk) / n - mean_j * mean_k
 *   (population moments; every fp64 operation rounded on its own, never an FMA); FLAT = 2^-6.
 *   k = 0: (1, 0).  k >= 1: with N >= 3, num = sum_j C_0j and den = sum_j C_kj over j not in {0, k}, ascending, from 0.0; where
 *   both are finite and >= FLAT, g = num / den (the cross rule: a third member's noise is independent of both).  Otherwise
 *   g = sqrt(C_00 / C_kk), or 1 where C_00 < FLAT, C_kk < FLAT or C_0k <= 0 (windows.align_solve's rule on the byte scale).
 *   g is clamped to [0.5, 2]; o = mean_0 - g * mean_k with the clamped g; anything non-finite: (1, 0); each rounded to fp32 once.
 * TWO launches, store-and-sum: every wave of a workgroup reduces fixed 8192-byte chunks of one clip to N + N (N + 1) / 2 unsigned
 * 32-bit partials (8192 * 255^2 < 2^32; byte products through v_dot4_u32_u8; 16 bytes per lane and member where every base and
 * clip_bytes are on the 16-byte grid, byte loads otherwise), at most 1024 workgroups of four waves per clip, further chunks a grid
 * stride on;
 * then one workgroup per clip adds the partials in 64-bit integers and evaluates the rule in fp64.  No atomics, no memset; all
 * sums are integers, so the bits do not depend on any order.  N = 1 writes (1, 0).
 * DRN_EINVAL (nothing launched): a null members, member, affine or workspace; N outside 1..16; B < 1 or > 65535; clip_bytes < 1 or
 * > 2^36 (every sum stays below 2^53 and converts to fp64 exactly); workspace_bytes too small; affine off the 4-byte grid; stats or
 * workspace off the 8-byte grid.  drn_ensemble_align_workspace_bytes: host arithmetic only; 0 for sizes the entry refuses. */
int64_t drn_ensemble_align_workspace_bytes(int N, int B, int64_t clip_bytes);
int drn_ensemble_align_affine(const void* const* members, int N, int B, int64_t clip_bytes, void* affine, void* stats,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* drn_ensemble_reduce_affine_u8: drn_ensemble_reduce_u8 in modes 0 and 1 with an affine in front: member k's byte x of clip b is
 * read as u8(rint(clamp(fp32(g * fp32(x)) + o, 0, 255))), (g, o) = affine[k][b] - two separately rounded fp32 operations (never
 * an FMA), the clamp, then half to even: torch's m.float() * g + o on the CPU -, and the median / mean and the spread are the
 * rules above on those bytes (the spread around the aligned members).  members: as above, uint8 [B * clip_bytes] each; affine:
 * fp32 [N][B][2] on the device, finite (every member's pair is applied, member 0's too); dst, spread: uint8 [B * clip_bytes],
 * spread or NULL.  (1, 0) gives the byte back: an all-identity affine gives drn_ensemble_reduce_u8's bits, and affine == NULL is
 * that entry on B * clip_bytes bytes.  ONE launch, one grid row per clip (a lane's 16 bytes never mix two clips' affines): 16 bytes
 * per lane where every base is 16-byte aligned and (B > 1) clip_bytes is a multiple of 16, one byte per lane otherwise - the same
 * bits; 64-bit offsets; the grid capped as in drn_ensemble_reduce_u8.
 * DRN_EINVAL (nothing launched): mode outside 0..1 (normal maps are never aligned); B < 1; clip_bytes < 0; affine off the 4-byte
 * grid; and the refusals of drn_ensemble_reduce_u8.  clip_bytes == 0: DRN_OK, nothing launched. */
int drn_ensemble_reduce_affine_u8(const void* const* members, int N, const void* affine, int B, int64_t clip_bytes, void* dst,
                                  void* spread, int mode, void* stream);

/* ---- relight edits: material edits and layer insertion on the device G-buffers, between the inverse and the forward stage of
 * Cosmos1Relight (no reference line: the reference has no such seam; the rule and the torch specification: gbuffer_edit.py,
 * edit_gbuffers).  ONE launch for all maps of a call.  maps: a HOST array of n_maps blocks (they travel to the
 * kernel by value: no device table); per map src, dst: uint8 [B][T][pixels][3]; layer: the inserted object's map, uint8 of the
 * same frame shape, or NULL; gain, offset: per channel, offsets on the byte scale; is_normal: the map holds encoded normals.
 * edit_mask: uint8 [B][T][pixels] or NULL (255 everywhere); insert_mask: the object's matte, likewise, needed with any layer
 * (without one it is not read).  Every tensor has a batch and a frame stride in BYTES, 0 = that axis is broadcast; a frame itself
 * is contiguous.  Per map, pixel and channel, with x = src's byte, m_e / m_i the pixel's mask bytes, L the layer's byte,
 * unit(i) = fp32(i) / 255.0f correctly rounded (fit.u8_unit), every fp32 operation rounded on its own, rint half to even:
 *   e = u8(rint(clamp(fp32(g * fp32(x)) + o, 0, 255)))        drn_ensemble_reduce_affine_u8's affine: two operations, never an FMA
 *   y = u8(rint(x + unit(m_e) * (e - x)))                     drn_tile_blend_u8's blend; m_e = 255 gives e, 0 gives x
 *   z = layer ? u8(rint(y + unit(m_i) * (L - y))) : y
 *   is_normal, a layer and m_i != 0:  z <- drn_ensemble_reduce_u8's mode 2 on the one pixel z (decode, renormalise, encode)
 * dst <- z.  A pixel with m_e == 0 and m_i == 0 keeps its bytes in every map; a normal is never renormalised where nothing was
 * inserted.  dst may be src (with src's strides: in place; a lane whose pixels all have both masks 0 then stores nothing);
 * otherwise it may overlap nothing.  Nothing outside dst is written.  16 whole pixels per lane (48 bytes of every map and layer,
 * 16 of every mask, in 16-byte words) where every base and every non-zero stride is on the 16-byte grid, with what pixels % 16
 * leaves of a frame one pixel per lane; one pixel per lane otherwise - the same bits.  64-bit offsets; the grid is capped at
 * 2048 blocks that stride over the flat (frame, piece) index.
 * DRN_EINVAL (nothing launched): a null maps, src or dst; n_maps outside 1..5; B < 1, T < 1, pixels < 0; a layer without
 * insert_mask; a non-finite gain or offset; a negative stride, a dst stride that lets two of its frames overlap, B T pixels
 * beyond 2^58; dst overlapping a mask, a layer, another map's src or dst, or its own src other than in place.  pixels == 0:
 * DRN_OK, nothing launched.  drn_gbuffer_edit_map_bytes: sizeof(drn_gbuffer_edit_map) as compiled (host only). */
typedef struct drn_gbuffer_edit_map {
    const void* src;
    void* dst;
    const void* layer;
    int64_t src_bs, src_ts, dst_bs, dst_ts, layer_bs, layer_ts;
    float gain[3], offset[3];
    int32_t is_normal;
    int32_t reserved;
} drn_gbuffer_edit_map;
int drn_gbuffer_edit_map_bytes(void);
int drn_gbuffer_edit_u8(const drn_gbuffer_edit_map* maps, int n_maps, const void* edit_mask, int64_t edit_mask_bs,
                        int64_t edit_mask_ts, const void* insert_mask, int64_t insert_mask_bs, int64_t insert_mask_ts, int B, int T,
                        int64_t pixels, void* stream);

/* ---- step cache (step_cache.py: the rule, the controller and the torch / numpy specification; no reference
 * counterpart).  A cached denoising loop runs block 0 on every step, asks how far the residual stream behind it moved since the
 * last computed step, and where it hardly moved adds that step's contribution of blocks 1 .. L-1 instead of running them.
 * Three streaming passes over [B][n] bf16 (n = S * D values per clip, contiguous), csrc/step_cache.hip:
 *
 * drn_step_cache_probe: stats [B][2] fp64 on the device = (num_b, den_b), num_b = sum_i |x_i - ref_i| with the subtraction ONE
 * rounded fp32 operation, den_b = sum_i |ref_i|, both summed in fp64 over clip b's n values.  Store-and-sum in the manner of
 * drn_window_align_affine, no atomics, no host read, the same bits run to run and at any alignment:
 *   chunk k of clip b = its values [8192 k, min(8192 (k + 1), n)); value j of a chunk (0 <= j < 8192) belongs to lane
 *   (j / 8) % 256; a lane adds its values in increasing j from 0.0; the 64 lanes of a wave are joined by the butterfly
 *   s_l <- s_l + s_(l ^ d) for d = 32, 16, 8, 4, 2, 1; the chunk's partial is ((w0 + w1) + w2) + w3 over its four waves (lanes
 *   0-63, 64-127, ...).  A second launch adds clip b's ceil(n / 8192) partials in index order: 64 contiguous runs of
 *   ceil(chunks / 64) partials, each from 0.0, then the runs in order from 0.0.  A NaN sum is stored as 0x7FF8000000000000.
 * Both bases 16-byte aligned and n % 8 == 0: 16-byte loads; otherwise 2-byte loads, in the SAME order (the same bits).  64-bit
 * offsets; the grid is capped at 2048 blocks that stride over the B * ceil(n / 8192) chunks.  workspace: at least
 * drn_step_cache_workspace_bytes(B, n) bytes (host arithmetic only; 0 for a non-positive size), 8-byte aligned, not initialised
 * by the caller.  DRN_EINVAL (nothing launched): a null x / ref / stats / workspace, a short workspace, B < 1, n < 1, x / ref off
 * 2 bytes, stats / workspace off 8.
 *
 * drn_step_cache_residual: r_i = bf16(fp32(x_i) - fp32(ref_i)); drn_step_cache_apply: x_i = bf16(fp32(x_i) + fp32(r_i)) in place.
 * Over n_total values, bit for bit torch's (a.float() -/+ b.float()).bfloat16(): one rounded fp32 operation, round to nearest
 * even, +-inf kept, every NaN result 0x7FC0 (c10's scalar conversion; torch's vectorised CPU loop writes 0xFFFF for the same
 * NaN, so against torch a NaN compares as a NaN).  Every base 16-byte aligned: 8 values per lane and the n_total % 8 tail one per lane;
 * otherwise one value per lane; 64-bit offsets, a capped grid that strides.  r may be x or ref.  DRN_EINVAL (nothing launched):
 * a null pointer, n_total < 1, a pointer off 2 bytes. */
int64_t drn_step_cache_workspace_bytes(int B, int64_t n);
int drn_step_cache_probe(const void* x, const void* ref, void* stats, void* workspace, int64_t workspace_bytes, int B, int64_t n,
                         void* stream);
int drn_step_cache_residual(const void* x, const void* ref, void* r, int64_t n_total, void* stream);
int drn_step_cache_apply(void* x, const void* r, int64_t n_total, void* stream);

/* =====================================================================================================
 * Cosmos-1.0 CV8x8x8 tokenizer (CleanVAE.py:45-60 -> diffusers.AutoencoderKLCosmos, un-vendored: parity unpinned).
 * Activations are channels-last bf16, X[t][h][w][c], stored with an optional 1-pixel zero halo in H and W
 * (`halo` = 0 compact / 1 padded); every kernel writes interior pixels only, so a zero-initialised halo stays zero.
 * ===================================================================================================== */

/* ---- causal conv3d as an implicit GEMM on MFMA (CosmosCausalConv3d / ConvProjection3d / 1x1x1 convs, and - with a
 * 1x1x1 kernel over a compact [M,K] matrix - the dense GEMMs of the mid-block attention).
 *   y[p, n] = bf16(bias[n] + sum x[in(p,tap), c] * w[n, tap*C + c]) (+ residual[p, n], rounded again)
 *   or, out_f32 != 0:  y_f32[p, n] = alpha * (bias[n] + sum ...)
 * x: [T][H+2*in_halo][W+2*in_halo][C]; w: [N][kT*kH*kW*C] (tap-major repack of the conv weight); bias: [N] or NULL;
 * y / residual: [To][Ho+2*out_halo][Wo+2*out_halo][ldc / ldr].  Input pixel of tap (kt,kh,kw) for output (to,ho,wo):
 *   t = max(to*sT + kt - t_off, 0) (causal replicate padding), h = ho*sH + kh - pad, w = wo*sW + kw - pad
 * (pad = 1 reads the zero halo).  C % 64 == 0, N % 4 == 0. */
int drn_conv3d_igemm(const void* x, const void* w, const void* bias, void* y, const void* residual,
                     int T, int H, int W, int C, int in_halo, int N,
                     int kT, int kH, int kW, int sT, int sH, int sW, int pad, int t_off,
                     int To, int Ho, int Wo, int out_halo, int64_t ldc, int64_t ldr,
                     int out_f32, float alpha, void* stream);
/* tuning hooks (no reference counterpart): the big convolutions (N % 256 == 0, bf16 output, >= 192 tiles of 256 positions x
 * 256 channels, input < 4 GiB) run on the streamed 256x256 kernel (csrc/conv256s.hip), everything else on the 128x128 one;
 * results are bit-identical.  drn_conv_force_tile: -1 automatic, 0 always 128x128, 1 256x256 wherever it can run;
 * drn_conv_last_tile: the kernel the last drn_conv3d_igemm call launched (0 / 1). */
void drn_conv_force_tile(int tile);
int drn_conv_last_tile(void);

/* ---- CosmosCausalGroupNorm(1 group, per frame) [+ SiLU]: y = [silu](bf16((x-mean)*rstd*gamma + beta)).
 * workspace: drn_groupnorm_workspace_bytes(frames) bytes of device scratch (0 for frames < 1, which the entry refuses). */
int drn_groupnorm_silu(const void* x, const void* gamma, const void* beta, void* y, void* workspace,
                       int frames, int H, int W, int C, int halo, float eps, int silu, void* stream);
int64_t drn_groupnorm_workspace_bytes(int frames);
/* the same normalisation in two steps, for frames whose rows are spread over several GPUs: per-rank
 * partial sums part[frames][64][2] as fp64 (sum, sum of squares over the stored band; the halo rows must still be zero; fp64 makes
 * the totals independent of the split), then - after the ranks' partials were gathered to part[frames][nparts][2] - the normalisation of this rank's band with
 * count = H_total * W * C elements per frame. */
int drn_groupnorm_stats(const void* x, void* part, int frames, int H, int W, int C, int halo, void* stream);
int drn_groupnorm_apply(const void* x, const void* part, int nparts, float count, const void* gamma, const void* beta,
                        void* y, int frames, int H, int W, int C, int halo, float eps, int silu, void* stream);

/* ---- 2-level 3-D Haar patching (CosmosPatchEmbed3d, patch 4): video [Cin][T][H][W] planar ->
 * [ (T+3)/4 ][H/4+2*halo][W/4+2*halo][64*Cin]; and its inverse (CosmosUnpatcher3d) -> [C][4*Tp-3][4*Hq][4*Wq]. */
int drn_haar_patch(const void* video, void* out, int Cin, int T, int H, int W, int halo, void* stream);
int drn_haar_unpatch(const void* patches, void* video, int Cimg, int Tp, int Hq, int Wq, int halo, void* stream);

/* ---- resampling helpers of CosmosDownsample3d / CosmosUpsample3d.  mode 0: spatial 2x2 mean, 1: causal temporal
 * 2-frame mean, 2: temporal nearest x2 minus the first frame, 3: spatial nearest x2. */
int drn_resample(const void* x, void* y, int mode, int T, int H, int W, int C, int To, int Ho, int Wo, int halo,
                 void* stream);

/* ---- mid-block attention pieces (1 head of dim C): fp32 row softmax -> bf16, bf16 transpose, causal temporal attention */
int drn_softmax_rows(const void* scores, void* probs, int64_t rows, int n, int64_t ld, int64_t ldp, void* stream);
/* the same with the scores multiplied by `scale` first (one fp32 product per element: what a GEMM epilogue with alpha = scale forms) */
int drn_softmax_rows_scaled(const void* scores, void* probs, int64_t rows, int n, int64_t ld, int64_t ldp, float scale, void* stream);
/* (transpose: ldo <= 65535 * 32 - the output rows' tiles are a grid dimension - and cols <= 2^31 - 32; temporal attention: at most
 * 2^33 - 4 pixels P, four per workgroup; DRN_EINVAL beyond, nothing launched) */
int drn_transpose_bf16(const void* x, void* y, int rows, int cols, int64_t ldx, int64_t ldo, void* stream);
int drn_temporal_attention(const void* q, const void* k, const void* v, void* o, int T, int64_t P, int C, float scale,
                           void* stream);

/* ---- latent layout moves: planar [C][T][H][W] <-> channels-last [T][H+2*halo][W+2*halo][Cs] (Cs >= C) */
int drn_planar_to_cl(const void* x, void* y, int C, int T, int H, int W, int Cs, int halo, void* stream);
int drn_cl_to_planar(const void* x, void* y, int C, int T, int H, int W, int Cs, int halo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRN_H */
