// HBM-bound token-local kernels of the DiT hot path and the sampler (gfx950, wave64).
// One read + one write of each activation row; all bf16 traffic is 16 B per lane.
// fp contraction is off in this file: several kernels are bit-exact restatements of unfused torch fp32 ops.
#pragma clang fp contract(off)
#include "drn_common.h"
#include "mx_quant.h"

// ------------------------------------------------------------------------------------------------
// LayerNorm (no affine) + AdaLN modulate, optional broadcast pre-add.
// CleanGeneralDIT.py:7-11, :481, :506, :517 (rounding points: SURVEY.md Appendix C).
//
// A row is NCH chunk columns of 64 lanes x 8 elements (chunk i of lane l = elements (l + 64 i) * 8 .. + 7).  Two kernels share ONE
// summation tree for the mean and the variance, so they return the same bits and the launcher may pick either by row count:
//     per lane and chunk: the 8 elements in order;  per lane and GROUP of NCH / 4 chunks: the chunks in order;
//     per group: the 64-lane butterfly;  total = (G0 + G1) + (G2 + G3).
//   * ln_modulate_kernel<NCH>:   one wave per row (a row stays in one wave's registers) - D <= 1024, the MXFP8 form with the
//     pre-add at many rows, and drn_ln_force_kernel(0);
//   * ln_modulate_kernel4<NCH>:  four waves per row, wave w owns group w, partial sums meet in LDS - few rows (cfg 1: 256 rows
//     on 64 workgroups of the one-wave kernel took 11.7 us per call, a chain of three memory round trips on a quarter of the CUs)
//     and many (18 432 rows: 7 waves per SIMD against 4, see launch_ln_modulate).
// NCH < 4 (D <= 1024: the tiny test networks) keeps a single butterfly and has no four-wave form.
// Where the modulated row goes.  MX = false: h [rows, D] bf16 (the kernels as they always were; hq / hs are unused trailing
// arguments).  MX = true: the same bf16 values quantised as MXFP8 (drn.h: elements hq [rows, D] + one E8M0 byte per 32 columns in
// hs), and h as well when it is not NULL.  A lane's 8 columns are a quarter of a 32-column block and the lanes l .. l ^ 3 hold the
// whole block (D % 32 == 0: the four are inside the row or outside it together): mx_quant_kernel's lane group, so the bytes are
// those of drn_mx_quant_bf16 on h.
template <bool MX>
__device__ __forceinline__ void ln_store(bf16_t* hr, uint8_t* hq, uint8_t* hs, int64_t row, int c, int D, const float (&o)[8]) {
    if (!MX) {
        *reinterpret_cast<uint4*>(hr + c) = pack8(o);
    } else {
        // the row is the same for the whole wave: as a scalar its three output addresses cost no VGPRs (as a vector value the
        // one-wave kernel at NCH = 4 took 70 VGPRs, 7 waves per SIMD against the bf16 form's 8)
        row = ((int64_t)__builtin_amdgcn_readfirstlane((int)(row >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)row);
        // o[] is bf16-exact (rounded through bf16 above): amax and elements straight from it, the packed row only for h
        uint32_t amax = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = max(amax, mx_abs_bits(o[j]));
        amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
        amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
        const int e = mx_block_exp(amax);
        const float inv = mx_inv_scale(e);
        if (hr) *reinterpret_cast<uint4*>(hr + c) = pack8(o);
        uint8_t* qrow = hq + row * D;                       // scalar bases + 32-bit lane offsets (saddr stores)
        uint8_t* srow = hs + row * (D / 32);
        *reinterpret_cast<uint2*>(qrow + (uint32_t)c) = make_uint2(mx_pack4f(o[0], o[1], o[2], o[3], inv), mx_pack4f(o[4], o[5], o[6], o[7], inv));
        if ((threadIdx.x & 3) == 0) srow[(uint32_t)c >> 5] = (uint8_t)(e + 127);
    }
}

template <int NCH>
__device__ __forceinline__ float ln_tree_sum(const float (&part)[NCH]) {
    if (NCH < 4) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) s += part[i];
        return wave_sum(s);
    }
    constexpr int G = NCH >= 4 ? NCH / 4 : 1;
    float g[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < G; ++i) t += part[(NCH >= 4 ? w * G : 0) + i];
        g[w] = t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                   // four independent butterflies, interleaved
#pragma unroll
        for (int w = 0; w < 4; ++w) g[w] += __shfl_xor(g[w], o, 64);
    }
    return (g[0] + g[1]) + (g[2] + g[3]);
}

template <int NCH, bool MX>
__global__ __launch_bounds__(256) void ln_modulate_kernel(bf16_t* __restrict__ x, const bf16_t* __restrict__ add,
                                                          const bf16_t* __restrict__ shift,
                                                          const bf16_t* __restrict__ scale, bf16_t* __restrict__ h,
                                                          int64_t rows, int D, int64_t rpb, float eps,
                                                          uint8_t* __restrict__ hq, uint8_t* __restrict__ hs) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / rpb;
    bf16_t* xr = x + row * D;
    const bf16_t* ar = add ? add + b * D : nullptr;
    float v[NCH][8];
    float part[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 8;
        float s = 0.f;
        if (c < D) {
            uint4 raw = *reinterpret_cast<const uint4*>(xr + c);
            unpack8(raw, v[i]);
            if (ar) {
                float a[8];
                unpack8(*reinterpret_cast<const uint4*>(ar + c), a);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = rbf(v[i][j] + a[j]);
                *reinterpret_cast<uint4*>(xr + c) = pack8(v[i]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[i][j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
        }
        part[i] = s;
    }
    const float mean = ln_tree_sum<NCH>(part) / (float)D;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 8;
        float q = 0.f;
        if (c < D) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[i][j] - mean;
                q += d * d;
            }
        }
        part[i] = q;
    }
    const float var = ln_tree_sum<NCH>(part) / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
    const bf16_t* sh = shift + b * D;
    const bf16_t* sc = scale + b * D;
    bf16_t* hr = (MX && !h) ? nullptr : h + row * D;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 8;
        if (c < D) {
            float fs[8], fc[8], o[8];
            unpack8(*reinterpret_cast<const uint4*>(sh + c), fs);
            unpack8(*reinterpret_cast<const uint4*>(sc + c), fc);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float n = rbf((v[i][j] - mean) * rstd);
                const float s1 = rbf(1.0f + fc[j]);
                o[j] = rbf(rbf(n * s1) + fs[j]);
            }
            ln_store<MX>(hr, hq, hs, row, c, D, o);
        }
    }
}

// four waves per row: wave w owns chunks w * G .. w * G + G - 1 (G = NCH / 4); D must fill all NCH chunk columns' lanes or leave
// whole lanes empty exactly as above (c < D test per chunk)
template <int NCH, bool MX>
__global__ __launch_bounds__(256) void ln_modulate_kernel4(bf16_t* __restrict__ x, const bf16_t* __restrict__ add,
                                                           const bf16_t* __restrict__ shift,
                                                           const bf16_t* __restrict__ scale, bf16_t* __restrict__ h,
                                                           int64_t rows, int D, int64_t rpb, float eps,
                                                           uint8_t* __restrict__ hq, uint8_t* __restrict__ hs) {
    static_assert(NCH >= 4 && NCH % 4 == 0, "four-wave form needs whole chunk groups");
    constexpr int G = NCH / 4;
    __shared__ float red[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    const int64_t b = row / rpb;
    bf16_t* xr = x + row * D;
    const bf16_t* ar = add ? add + b * D : nullptr;
    const bf16_t* sh = shift + b * D;
    const bf16_t* sc = scale + b * D;
    float v[G][8], fs[G][8], fc[G][8];
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = (lane + 64 * (w * G + g)) * 8;
        float s = 0.f;
        if (c < D) {
            unpack8(*reinterpret_cast<const uint4*>(xr + c), v[g]);
            unpack8(*reinterpret_cast<const uint4*>(sh + c), fs[g]);     // (independent of the statistics: in flight with the row)
            unpack8(*reinterpret_cast<const uint4*>(sc + c), fc[g]);
            if (ar) {
                float a[8];
                unpack8(*reinterpret_cast<const uint4*>(ar + c), a);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[g][j] = rbf(v[g][j] + a[j]);
                *reinterpret_cast<uint4*>(xr + c) = pack8(v[g]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[g][j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[g][j] = 0.f;
        }
        t += s;
    }
    t = wave_sum(t);
    if (lane == 0) red[0][w] = t;
    __syncthreads();
    const float mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)D;
    float tq = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = (lane + 64 * (w * G + g)) * 8;
        float q = 0.f;
        if (c < D) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[g][j] - mean;
                q += d * d;
            }
        }
        tq += q;
    }
    tq = wave_sum(tq);
    if (lane == 0) red[1][w] = tq;
    __syncthreads();
    const float var = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
    bf16_t* hr = (MX && !h) ? nullptr : h + row * D;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = (lane + 64 * (w * G + g)) * 8;
        if (c < D) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float n = rbf((v[g][j] - mean) * rstd);
                const float s1 = rbf(1.0f + fc[g][j]);
                o[j] = rbf(rbf(n * s1) + fs[g][j]);
            }
            ln_store<MX>(hr, hq, hs, row, c, D, o);
        }
    }
}

// Split-K sum + gated residual + the NEXT sub-block's LayerNorm / modulate in one pass (few-token shapes: cfg 1 ran
// gemm_splitk_epilogue_kernel<2> and ln_modulate back to back on 2 MB of activations, ~9 us + ~6 us + a launch gap, 56 times per forward):
//   a     = part[0][row] + part[1][row] + ...            fp32, slices in order        (= gemm_splitk_epilogue_kernel)
//   x     = bf16(x + bf16(gate * bf16(a)))               written back                 (= its DRN_EPI_GATE_RES epilogue)
//   x     = bf16(x + add_vec) if add_vec                 written back instead         (= ln_modulate's broadcast pre-add)
//   h     = modulate(LayerNorm(x))                       four waves per row           (= ln_modulate_kernel4: same summation tree)
// Every step rounds where the separate kernels round: the same bits as epilogue kernel + ln_modulate.
template <int NCH, bool MX>
__global__ __launch_bounds__(256) void splitk_gate_res_ln_kernel(const float* __restrict__ part, int splits, int64_t part_stride,
                                                                 bf16_t* __restrict__ x, const bf16_t* __restrict__ gate,
                                                                 const bf16_t* __restrict__ add, const bf16_t* __restrict__ shift,
                                                                 const bf16_t* __restrict__ scale, bf16_t* __restrict__ h,
                                                                 int D, int64_t rpb, float eps,
                                                                 uint8_t* __restrict__ hq, uint8_t* __restrict__ hs) {
    static_assert(NCH >= 4 && NCH % 4 == 0, "four waves per row");
    constexpr int G = NCH / 4;
    __shared__ float red[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    const int64_t b = row / rpb;
    bf16_t* xr = x + row * D;
    const float* pr = part + row * D;
    const bf16_t* gr = gate + b * D;
    const bf16_t* ar = add ? add + b * D : nullptr;
    const bf16_t* sh = shift + b * D;
    const bf16_t* sc = scale + b * D;
    float v[G][8], fs[G][8], fc[G][8];
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = (lane + 64 * (w * G + g)) * 8;
        float s = 0.f;
        if (c < D) {
            // slices summed in order (as gemm_splitk_epilogue_kernel), loaded four at a time: eight 16-byte loads in flight
            f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(pr + c), a1 = *reinterpret_cast<const f32x4_t*>(pr + c + 4);
            int sp = 1;
            for (; sp + 4 <= splits; sp += 4) {
                f32x4_t l0[4], l1[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    l0[u] = *reinterpret_cast<const f32x4_t*>(pr + (sp + u) * part_stride + c);
                    l1[u] = *reinterpret_cast<const f32x4_t*>(pr + (sp + u) * part_stride + c + 4);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a0 += l0[u];
                    a1 += l1[u];
                }
            }
            for (; sp < splits; ++sp) {
                a0 += *reinterpret_cast<const f32x4_t*>(pr + sp * part_stride + c);
                a1 += *reinterpret_cast<const f32x4_t*>(pr + sp * part_stride + c + 4);
            }
            float xv[8], gv[8];
            unpack8(*reinterpret_cast<const uint4*>(xr + c), xv);
            unpack8(*reinterpret_cast<const uint4*>(gr + c), gv);
            unpack8(*reinterpret_cast<const uint4*>(sh + c), fs[g]);
            unpack8(*reinterpret_cast<const uint4*>(sc + c), fc[g]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float acc = j < 4 ? a0[j] : a1[j - 4];
                v[g][j] = rbf(xv[j] + rbf(gv[j] * rbf(acc)));
            }
            if (ar) {
                float a[8];
                unpack8(*reinterpret_cast<const uint4*>(ar + c), a);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[g][j] = rbf(v[g][j] + a[j]);
            }
            *reinterpret_cast<uint4*>(xr + c) = pack8(v[g]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[g][j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[g][j] = 0.f;
        }
        t += s;
    }
    t = wave_sum(t);
    if (lane == 0) red[0][w] = t;
    __syncthreads();
    const float mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)D;
    float tq = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = (lane + 64 * (w * G + g)) * 8;
        float q = 0.f;
        if (c < D) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[g][j] - mean;
                q += d * d;
            }
        }
        tq += q;
    }
    tq = wave_sum(tq);
    if (lane == 0) red[1][w] = tq;
    __syncthreads();
    const float var = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
    bf16_t* hr = (MX && !h) ? nullptr : h + row * D;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = (lane + 64 * (w * G + g)) * 8;
        if (c < D) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float n = rbf((v[g][j] - mean) * rstd);
                const float s1 = rbf(1.0f + fc[g][j]);
                o[j] = rbf(rbf(n * s1) + fs[g][j]);
            }
            ln_store<MX>(hr, hq, hs, row, c, D, o);
        }
    }
}

template <bool MX>
static int launch_splitk_gate_res_ln(const void* partials, int splits, void* x, const void* gate, const void* add_vec,
                                     const void* shift, const void* scale, void* h, void* hq, void* hs, int64_t rows, int64_t D,
                                     int64_t rows_per_batch, float eps, void* stream) {
    DRN_CHECK_ARG(partials && x && gate && shift && scale && splits >= 1 && rows >= 0 && rows < (1ll << 31));
    DRN_CHECK_ARG(D > 1024 && D % 8 == 0 && D <= 8192 && rows_per_batch > 0 && ((uintptr_t)partials & 15) == 0);
    if (rows == 0) return DRN_OK;
    const int nch = (int)((D + 511) / 512);
    dim3 grid((unsigned)rows), block(256);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(N)                                                                                                     \
    splitk_gate_res_ln_kernel<N, MX><<<grid, block, 0, st>>>((const float*)partials, splits, rows * D, (bf16_t*)x,   \
        (const bf16_t*)gate, (const bf16_t*)add_vec, (const bf16_t*)shift, (const bf16_t*)scale, (bf16_t*)h, (int)D,  \
        rows_per_batch, eps, (uint8_t*)hq, (uint8_t*)hs)
    if (nch <= 4) LAUNCH(4);
    else if (nch <= 8) LAUNCH(8);
    else LAUNCH(16);
#undef LAUNCH
    return drn_launch_status();
}

extern "C" int drn_splitk_gate_res_ln_modulate(const void* partials, int splits, void* x, const void* gate, const void* add_vec,
                                               const void* shift, const void* scale, void* h, int64_t rows, int64_t D,
                                               int64_t rows_per_batch, float eps, void* stream) {
    DRN_CHECK_ARG(h);
    return launch_splitk_gate_res_ln<false>(partials, splits, x, gate, add_vec, shift, scale, h, nullptr, nullptr, rows, D,
                                            rows_per_batch, eps, stream);
}

extern "C" int drn_splitk_gate_res_ln_modulate_mx(const void* partials, int splits, void* x, const void* gate, const void* add_vec,
                                                  const void* shift, const void* scale, void* h, void* hq, void* hs, int64_t rows,
                                                  int64_t D, int64_t rows_per_batch, float eps, void* stream) {
    DRN_CHECK_ARG(hq && hs && D % 32 == 0 && ((uintptr_t)hq & 7) == 0);
    return launch_splitk_gate_res_ln<true>(partials, splits, x, gate, add_vec, shift, scale, h, hq, hs, rows, D, rows_per_batch, eps,
                                           stream);
}

static int g_ln_force = -1;      // tests: 0 = one wave per row always, 1 = four waves per row wherever it exists, -1 = by row count
extern "C" void drn_ln_force_kernel(int which) { g_ln_force = which; }

template <bool MX>
static int launch_ln_modulate(void* x, const void* add_vec, const void* shift, const void* scale, void* h, void* hq, void* hs,
                              int64_t rows, int64_t D, int64_t rows_per_batch, float eps, void* stream) {
    DRN_CHECK_ARG(x && shift && scale && rows >= 0 && D > 0 && D % 8 == 0 && D <= 8192 && rows_per_batch > 0);
    DRN_CHECK_ARG((rows + 3) / 4 < (1ll << 31));                         // one workgroup index in 31 bits (four rows per workgroup)
    if (rows == 0) return DRN_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nch = (int)((D + 511) / 512);
    // four waves per row (same bits as one wave per row: shared summation tree) - 4 x the waves in flight: few rows, and many rows
    // too (18432 x 4096, tools/lnbench.py over rotating buffers, profiles/harvest_18k.txt 3: without the pre-add 79.6 us one wave
    // per row, 58.4 four; with it 105.7 vs 95.6 us - on one buffer pair, which the Infinity Cache then holds, that pair was a
    // draw).  The MXFP8 form with the pre-add at many rows keeps the one-wave kernel: nobody measured it.  D <= 1024 has one form.
    const bool four = nch > 2 && rows < (1ll << 31) && (g_ln_force == 1 || (g_ln_force < 0 && (rows <= 4096 || !add_vec || !MX)));
    dim3 grid(four ? (unsigned)rows : (unsigned)((rows + 3) / 4)), block(256);
#define LAUNCH(K, N)                                                                                                  \
    K<N, MX><<<grid, block, 0, st>>>((bf16_t*)x, (const bf16_t*)add_vec, (const bf16_t*)shift, (const bf16_t*)scale,  \
                                     (bf16_t*)h, rows, (int)D, rows_per_batch, eps, (uint8_t*)hq, (uint8_t*)hs)
    if (nch <= 1) LAUNCH(ln_modulate_kernel, 1);
    else if (nch <= 2) LAUNCH(ln_modulate_kernel, 2);
    else if (nch <= 4) { if (four) LAUNCH(ln_modulate_kernel4, 4); else LAUNCH(ln_modulate_kernel, 4); }
    else if (nch <= 8) { if (four) LAUNCH(ln_modulate_kernel4, 8); else LAUNCH(ln_modulate_kernel, 8); }
    else { if (four) LAUNCH(ln_modulate_kernel4, 16); else LAUNCH(ln_modulate_kernel, 16); }
#undef LAUNCH
    return drn_launch_status();
}

extern "C" int drn_ln_modulate(void* x, const void* add_vec, const void* shift, const void* scale, void* h,
                               int64_t rows, int64_t D, int64_t rows_per_batch, float eps, void* stream) {
    DRN_CHECK_ARG(h);
    return launch_ln_modulate<false>(x, add_vec, shift, scale, h, nullptr, nullptr, rows, D, rows_per_batch, eps, stream);
}

extern "C" int drn_ln_modulate_mx(void* x, const void* add_vec, const void* shift, const void* scale, void* h, void* hq, void* hs,
                                  int64_t rows, int64_t D, int64_t rows_per_batch, float eps, void* stream) {
    DRN_CHECK_ARG(hq && hs && D % 32 == 0 && ((uintptr_t)hq & 7) == 0);
    return launch_ln_modulate<true>(x, add_vec, shift, scale, h, hq, hs, rows, D, rows_per_batch, eps, stream);
}

// ------------------------------------------------------------------------------------------------
// x[rows, D] <- bf16(x + vec[batch])   (broadcast cross-attention residual, CleanGeneralDIT.py:517 + F8)
__global__ __launch_bounds__(256) void bcast_add_kernel(bf16_t* __restrict__ x, const bf16_t* __restrict__ vec,
                                                        int64_t nchunks, int dchunks, int64_t rpb) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / dchunks;
        const int c = (int)(i - row * dchunks);
        const int64_t b = row / rpb;
        float a[8], v[8];
        unpack8(*reinterpret_cast<const uint4*>(x + i * 8), v);
        unpack8(*reinterpret_cast<const uint4*>(vec + (b * dchunks + c) * 8), a);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = rbf(v[j] + a[j]);
        *reinterpret_cast<uint4*>(x + i * 8) = pack8(v);
    }
}

extern "C" int drn_bcast_add(void* x, const void* vec, int64_t rows, int64_t D, int64_t rows_per_batch, void* stream) {
    DRN_CHECK_ARG(x && vec && rows >= 0 && D > 0 && D % 8 == 0 && rows_per_batch > 0);
    if (rows == 0) return DRN_OK;
    const int64_t nchunks = rows * (D / 8);
    int64_t blocks = (nchunks + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    bcast_add_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>((bf16_t*)x, (const bf16_t*)vec,
                                                                                    nchunks, (int)(D / 8), rows_per_batch);
    return drn_launch_status();
}

// ------------------------------------------------------------------------------------------------
// y[b][a][:] = x[a][b][:], 16-byte chunks (regroup around the sequence-parallel all-to-all; C >= 512 in practice, so every
// run of C elements is a coalesced >= 1 KB read and write)
__global__ __launch_bounds__(256) void permute_021_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int64_t A,
                                                          int64_t B, int64_t cch) {
    const int64_t n = A * B * cch;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i % cch;
        const int64_t ba = i / cch;           // = b * A + a  (output order)
        const int64_t a = ba % A, b = ba / A;
        y[i] = x[(a * B + b) * cch + c];
    }
}

extern "C" int drn_permute_021(const void* x, void* y, int64_t A, int64_t B, int64_t C, void* stream) {
    DRN_CHECK_ARG(x && y && x != y && A >= 0 && B >= 0 && C > 0 && C % 8 == 0);
    DRN_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0);
    const int64_t n = A * B * (C / 8);
    if (n == 0) return DRN_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    permute_021_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>((const uint4*)x, (uint4*)y, A, B, C / 8);
    return drn_launch_status();
}

// ------------------------------------------------------------------------------------------------
// RMSNorm over the last dim (CleanGeneralDIT.py:14-33).  One wave per row, any D % 8 == 0.
__global__ __launch_bounds__(256) void rmsnorm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                      bf16_t* __restrict__ y, int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bf16_t* xr = x + row * D;
    float s = 0.f;
    for (int c = lane * 8; c < D; c += 512) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(xr + c), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j] * v[j];
    }
    const float r = 1.0f / sqrtf(wave_sum(s) / (float)D + eps);
    bf16_t* yr = y + row * D;
    for (int c = lane * 8; c < D; c += 512) {
        float v[8], g[8];
        unpack8(*reinterpret_cast<const uint4*>(xr + c), v);
        unpack8(*reinterpret_cast<const uint4*>(w + c), g);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (v[j] * r) * g[j];
        *reinterpret_cast<uint4*>(yr + c) = pack8(v);
    }
}

extern "C" int drn_rmsnorm(const void* x, const void* w, void* y, int64_t rows, int64_t D, float eps, void* stream) {
    DRN_CHECK_ARG(x && w && y && rows >= 0 && D > 0 && D % 8 == 0);
    DRN_CHECK_ARG(D < (1ll << 31) && (rows + 3) / 4 < (1ll << 31));     // the kernel's int D; one workgroup index in 31 bits
    if (rows == 0) return DRN_OK;
    rmsnorm_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
        (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, rows, (int)D, eps);
    return drn_launch_status();
}

// ------------------------------------------------------------------------------------------------
// per-head RMSNorm(q,k) + RoPE, in place.  8 lanes per 128-wide head row (lane j owns elements 8j..8j+7 and
// 64+8j..64+8j+7, i.e. both members of every rotate_half pair), 8 head rows per wave.
// CleanGeneralDIT.py:288-295 (norm), :45-84 (RoPE; cos/sin tables are host-built bf16).
// MX = true (a second instantiation: the bf16 one is untouched): the result is (also) written as MXFP8, QQ | QS and KQ | KS contiguous
// [tokens, heads * 128] e4m3 + [tokens, heads * 4] scales (drn.h: the bytes of drn_mx_quant_bf16 on what the bf16 form writes); the
// in-place bf16 result only when write_bf16.  A 32-element block is the lo (or hi) halves of the four lanes j .. j ^ 3.
template <bool MX>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(bf16_t* __restrict__ q, bf16_t* __restrict__ k,
                                                           const bf16_t* __restrict__ wq, const bf16_t* __restrict__ wk,
                                                           const bf16_t* __restrict__ cs, const bf16_t* __restrict__ sn,
                                                           int64_t tokens, int heads, int64_t ldq, int64_t ldk,
                                                           int64_t tpb, int64_t pos_offset, float eps,
                                                           uint8_t* __restrict__ QQ, uint8_t* __restrict__ QS,
                                                           uint8_t* __restrict__ KQ, uint8_t* __restrict__ KS, int write_bf16) {
    const int lane = threadIdx.x & 63;
    const int hr = lane >> 3, j = lane & 7;
    const int hgroups = (heads + 7) / 8;
    const int nwhich = (q ? 1 : 0) + (k ? 1 : 0);          // either tensor may be NULL (q and k handled by separate calls)
    const int64_t items = tokens * hgroups * nwhich;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t it = wave0; it < items; it += nwaves) {
        const int which = nwhich == 2 ? (int)(it & 1) : (q ? 0 : 1);
        const int64_t r = nwhich == 2 ? (it >> 1) : it;
        const int64_t tok = r / hgroups;
        const int head = (int)(r - tok * hgroups) * 8 + hr;
        const bool act = head < heads;
        bf16_t* base = (which ? k + tok * ldk : q + tok * ldq) + (int64_t)head * 128;
        const bf16_t* w = which ? wk : wq;
        float lo[8], hi[8];
        if (act) {
            unpack8(*reinterpret_cast<const uint4*>(base + 8 * j), lo);
            unpack8(*reinterpret_cast<const uint4*>(base + 64 + 8 * j), hi);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) lo[i] = hi[i] = 0.f;
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += lo[i] * lo[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += hi[i] * hi[i];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        const float rinv = 1.0f / sqrtf(s / 128.0f + eps);
        float wl[8], wh[8];
        unpack8(*reinterpret_cast<const uint4*>(w + 8 * j), wl);
        unpack8(*reinterpret_cast<const uint4*>(w + 64 + 8 * j), wh);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            lo[i] = rbf((lo[i] * rinv) * wl[i]);
            hi[i] = rbf((hi[i] * rinv) * wh[i]);
        }
        if (cs) {
            const int64_t p = pos_offset + (tok % tpb);
            float cl[8], ch[8], sl[8], sh[8];
            unpack8(*reinterpret_cast<const uint4*>(cs + p * 128 + 8 * j), cl);
            unpack8(*reinterpret_cast<const uint4*>(cs + p * 128 + 64 + 8 * j), ch);
            unpack8(*reinterpret_cast<const uint4*>(sn + p * 128 + 8 * j), sl);
            unpack8(*reinterpret_cast<const uint4*>(sn + p * 128 + 64 + 8 * j), sh);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float a = lo[i], b = hi[i];
                lo[i] = rbf(rbf(a * cl[i]) + rbf((-b) * sl[i]));
                hi[i] = rbf(rbf(b * ch[i]) + rbf(a * sh[i]));
            }
        }
        if (MX) {
            uint32_t al = 0, ah = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                al = max(al, mx_abs_bits(lo[i]));
                ah = max(ah, mx_abs_bits(hi[i]));
            }
            al = max(al, (uint32_t)__shfl_xor((int)al, 1, 64));
            ah = max(ah, (uint32_t)__shfl_xor((int)ah, 1, 64));
            al = max(al, (uint32_t)__shfl_xor((int)al, 2, 64));
            ah = max(ah, (uint32_t)__shfl_xor((int)ah, 2, 64));
            const int el = mx_block_exp(al), eh = mx_block_exp(ah);
            const float il = mx_inv_scale(el), ih = mx_inv_scale(eh);
            if (act) {
                const int64_t r = tok * heads + head;
                uint8_t* eq = (which ? KQ : QQ) + r * 128;
                uint8_t* es = (which ? KS : QS) + r * 4;
                *reinterpret_cast<uint2*>(eq + 8 * j) =
                    make_uint2(mx_pack4f(lo[0], lo[1], lo[2], lo[3], il), mx_pack4f(lo[4], lo[5], lo[6], lo[7], il));
                *reinterpret_cast<uint2*>(eq + 64 + 8 * j) =
                    make_uint2(mx_pack4f(hi[0], hi[1], hi[2], hi[3], ih), mx_pack4f(hi[4], hi[5], hi[6], hi[7], ih));
                if ((j & 3) == 0) {
                    es[j >> 2] = (uint8_t)(el + 127);
                    es[2 + (j >> 2)] = (uint8_t)(eh + 127);
                }
            }
        }
        if (act && (!MX || write_bf16)) {
            *reinterpret_cast<uint4*>(base + 8 * j) = pack8(lo);
            *reinterpret_cast<uint4*>(base + 64 + 8 * j) = pack8(hi);
        }
    }
}

extern "C" int drn_qk_norm_rope(void* q, void* k, const void* wq, const void* wk, const void* cos, const void* sin,
                                int64_t tokens, int heads, int64_t ldq, int64_t ldk, int64_t tokens_per_batch,
                                int64_t pos_offset, float eps, void* stream) {
    DRN_CHECK_ARG((q || k) && (!q || wq) && (!k || wk) && tokens >= 0 && heads > 0 && ldq % 8 == 0 && ldk % 8 == 0 &&
                  tokens_per_batch > 0);
    DRN_CHECK_ARG((cos == nullptr) == (sin == nullptr));
    if (tokens == 0) return DRN_OK;
    const int64_t items = tokens * ((heads + 7) / 8) * ((q ? 1 : 0) + (k ? 1 : 0));
    int64_t blocks = (items + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    qk_norm_rope_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(
        (bf16_t*)q, (bf16_t*)k, (const bf16_t*)wq, (const bf16_t*)wk, (const bf16_t*)cos, (const bf16_t*)sin, tokens,
        heads, ldq, ldk, tokens_per_batch, pos_offset, eps, nullptr, nullptr, nullptr, nullptr, 1);
    return drn_launch_status();
}

extern "C" int drn_qk_norm_rope_mx(void* q, void* k, const void* wq, const void* wk, const void* cos, const void* sin, void* qq,
                                   void* qs, void* kq, void* ks, int64_t tokens, int heads, int64_t ldq, int64_t ldk,
                                   int64_t tokens_per_batch, int64_t pos_offset, float eps, int write_bf16, void* stream) {
    DRN_CHECK_ARG((q || k) && (!q || (wq && qq && qs)) && (!k || (wk && kq && ks)) && tokens >= 0 && heads > 0 && ldq % 8 == 0 &&
                  ldk % 8 == 0 && tokens_per_batch > 0 && (write_bf16 == 0 || write_bf16 == 1));
    DRN_CHECK_ARG((cos == nullptr) == (sin == nullptr));
    DRN_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)qq & 7) == 0 && ((uintptr_t)kq & 7) == 0);
    if (tokens == 0) return DRN_OK;
    const int64_t items = tokens * ((heads + 7) / 8) * ((q ? 1 : 0) + (k ? 1 : 0));
    int64_t blocks = (items + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    qk_norm_rope_kernel<true><<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(
        (bf16_t*)q, (bf16_t*)k, (const bf16_t*)wq, (const bf16_t*)wk, (const bf16_t*)cos, (const bf16_t*)sin, tokens,
        heads, ldq, ldk, tokens_per_batch, pos_offset, eps, (uint8_t*)qq, (uint8_t*)qs, (uint8_t*)kq, (uint8_t*)ks, write_bf16);
    return drn_launch_status();
}

// ------------------------------------------------------------------------------------------------
// patchify + concat [x | cond | ones] -> token rows (c r m n), zero K-padding.  CleanGeneralDIT.py:669-675, :409-414.
__global__ __launch_bounds__(256) void patchify_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ cond,
                                                       bf16_t* __restrict__ out, int B, int Cx, int Cc, int with_mask,
                                                       int Tl, int Hl, int Wl, int pt, int ps, int64_t ldo) {
    const int Tp = Tl / pt, Hp = Hl / ps, Wp = Wl / ps;
    const int C = Cx + Cc + (with_mask ? 1 : 0);
    const int kdim = C * pt * ps * ps;
    const int64_t total = (int64_t)B * Tp * Hp * Wp * ldo;
    const int64_t plane = (int64_t)Tl * Hl * Wl;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t tokrow = i / ldo;
        const int col = (int)(i - tokrow * ldo);
        bf16_t val = 0;
        if (col < kdim) {
            int n = col % ps;
            int m = (col / ps) % ps;
            int r = (col / (ps * ps)) % pt;
            int c = col / (ps * ps * pt);
            int64_t t = tokrow;
            const int w = (int)(t % Wp); t /= Wp;
            const int hh = (int)(t % Hp); t /= Hp;
            const int tt = (int)(t % Tp);
            const int b = (int)(t / Tp);
            const int64_t sp = ((int64_t)(tt * pt + r) * Hl + (hh * ps + m)) * Wl + (w * ps + n);
            if (c < Cx) val = x[((int64_t)b * Cx + c) * plane + sp];
            else if (c < Cx + Cc) val = cond[((int64_t)b * Cc + (c - Cx)) * plane + sp];
            else val = 0x3F80;   // 1.0 (padding mask, CleanGeneralDIT.py:672)
        }
        out[i] = val;
    }
}

extern "C" int drn_patchify_concat(const void* x, const void* cond, void* out, int B, int Cx, int Cc, int with_mask,
                                   int Tl, int Hl, int Wl, int pt, int ps, int64_t ldo, void* stream) {
    DRN_CHECK_ARG(x && out && B > 0 && Cx > 0 && Cc >= 0 && (Cc == 0 || cond) && pt > 0 && ps > 0);
    DRN_CHECK_ARG(Tl > 0 && Hl > 0 && Wl > 0);                           // (an empty latent would be a launch of zero workgroups)
    DRN_CHECK_ARG(Tl % pt == 0 && Hl % ps == 0 && Wl % ps == 0);
    DRN_CHECK_ARG(ldo >= (int64_t)(Cx + Cc + (with_mask ? 1 : 0)) * pt * ps * ps);
    const int64_t total = (int64_t)B * (Tl / pt) * (Hl / ps) * (Wl / ps) * ldo;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    patchify_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(
        (const bf16_t*)x, (const bf16_t*)cond, (bf16_t*)out, B, Cx, Cc, with_mask, Tl, Hl, Wl, pt, ps, ldo);
    return drn_launch_status();
}

// unpatchify '(B T)(H W)(ph pw pt C) -> B C (T pt)(H ph)(W pw)', CleanGeneralDIT.py:709-716
__global__ __launch_bounds__(256) void unpatchify_kernel(const bf16_t* __restrict__ y, int64_t ldy,
                                                         bf16_t* __restrict__ out, int B, int C, int Tp, int Hp, int Wp,
                                                         int pt, int ps) {
    const int To = Tp * pt, Ho = Hp * ps, Wo = Wp * ps;
    const int64_t total = (int64_t)B * C * To * Ho * Wo;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t t = i;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho); t /= Ho;
        const int to = (int)(t % To); t /= To;
        const int c = (int)(t % C);
        const int b = (int)(t / C);
        const int W = wo / ps, pw = wo % ps, H = ho / ps, ph = ho % ps, T = to / pt, ptt = to % pt;
        const int64_t tokrow = (((int64_t)b * Tp + T) * Hp + H) * Wp + W;
        const int col = ((ph * ps + pw) * pt + ptt) * C + c;
        out[i] = y[tokrow * ldy + col];
    }
}

extern "C" int drn_unpatchify(const void* y, int64_t ldy, void* out, int B, int C, int Tp, int Hp, int Wp, int pt,
                              int ps, void* stream) {
    DRN_CHECK_ARG(y && out && B > 0 && C > 0 && Tp > 0 && Hp > 0 && Wp > 0 && pt > 0 && ps > 0);
    DRN_CHECK_ARG(ldy >= (int64_t)C * pt * ps * ps);
    const int64_t total = (int64_t)B * C * Tp * pt * Hp * ps * Wp * ps;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    unpatchify_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>((const bf16_t*)y, ldy,
                                                                                     (bf16_t*)out, B, C, Tp, Hp, Wp, pt, ps);
    return drn_launch_status();
}

// ------------------------------------------------------------------------------------------------
// EDM Euler sampler, model_diffusion_renderer.py:30-82.  Scalars are computed on the host with the reference's
// own fp32 torch ops; the kernels repeat its unfused fp32 elementwise sequence, so results are bit-exact.
__global__ __launch_bounds__(256) void edm_scale_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ o, int64_t n,
                                                        float c_in) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        o[i] = f2bf(bf2f(x[i]) * c_in);
}
__global__ __launch_bounds__(256) void edm_step_kernel(const bf16_t* __restrict__ mo, const bf16_t* __restrict__ x,
                                                       bf16_t* __restrict__ o, int64_t n, float c_skip, float c_out,
                                                       float sigma, float dt) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float sm = bf2f(x[i]);
        const float m = bf2f(mo[i]);
        const float denoised = c_skip * sm + c_out * m;
        const float deriv = (sm - denoised) / sigma;
        o[i] = f2bf(sm + deriv * dt);
    }
}
// CFG: out = bf16(c + bf16(g * bf16(c - u)))   model_diffusion_renderer.py:232
__global__ __launch_bounds__(256) void cfg_kernel(const bf16_t* __restrict__ c, const bf16_t* __restrict__ u,
                                                  bf16_t* __restrict__ o, int64_t n, float g) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float cc = bf2f(c[i]);
        const float d = rbf(cc - bf2f(u[i]));
        o[i] = f2bf(cc + rbf(g * d));
    }
}
static inline dim3 ew_grid(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return dim3((unsigned)b);
}
extern "C" int drn_edm_scale_input(const void* x, void* out, int64_t n, float c_in, void* stream) {
    DRN_CHECK_ARG(x && out && n >= 0);
    if (n == 0) return DRN_OK;
    edm_scale_kernel<<<ew_grid(n), dim3(256), 0, (hipStream_t)stream>>>((const bf16_t*)x, (bf16_t*)out, n, c_in);
    return drn_launch_status();
}
extern "C" int drn_edm_step(const void* model_out, const void* sample, void* out, int64_t n, float c_skip, float c_out,
                            float sigma, float dt, void* stream) {
    DRN_CHECK_ARG(model_out && sample && out && n >= 0);
    if (n == 0) return DRN_OK;
    edm_step_kernel<<<ew_grid(n), dim3(256), 0, (hipStream_t)stream>>>((const bf16_t*)model_out, (const bf16_t*)sample,
                                                                       (bf16_t*)out, n, c_skip, c_out, sigma, dt);
    return drn_launch_status();
}
extern "C" int drn_cfg_combine(const void* cond, const void* uncond, void* out, int64_t n, float guidance, void* stream) {
    DRN_CHECK_ARG(cond && uncond && out && n >= 0);
    if (n == 0) return DRN_OK;
    cfg_kernel<<<ew_grid(n), dim3(256), 0, (hipStream_t)stream>>>((const bf16_t*)cond, (const bf16_t*)uncond,
                                                                  (bf16_t*)out, n, guidance);
    return drn_launch_status();
}

// ------------------------------------------------------------------------------------------------
// pipeline post-process -> uint8 (B,T,H,W,3); diffusion_renderer_pipeline.py:299-318 with every bf16 rounding kept.
// One pixel's chain is postprocess_pixel, and the ramp's cross-fade window_blend, both in drn_common.h (window_align.hip shares them).

// ------------------------------------------------------------------------------------------------
// post-process of one WINDOW of a long clip (drn.h): frames [write_lo, write_hi) of the decoded window -> uint8, the O ramp frames
// cross-faded in fp32 with the previous window's last O decoded frames before the chain above.  A block works inside ONE output
// frame (blockIdx.y strides the B * (write_hi - write_lo) frames), so "is this a ramp frame" and its weight are uniform.
// VEC: a lane owns 8 consecutive pixels of the frame - one 16-byte load per channel plane (two on a ramp frame) and 24 contiguous
// output bytes as three 8-byte stores, a wave writes 1536 contiguous bytes.  Needs H * W % 8 == 0 (every plane of every frame then
// starts 16-byte aligned, and a frame is whole groups: no partial group exists); any other shape takes the one-pixel-per-lane form.
template <bool VEC>
__global__ __launch_bounds__(256) void postprocess_window_kernel(const bf16_t* __restrict__ v, const bf16_t* __restrict__ prev,
                                                                 const float* __restrict__ rw, uint8_t* __restrict__ o,
                                                                 int nframes, int nF, int Tw, int64_t hw, int O, int ramp_at,
                                                                 int write_lo, int normalize) {
    for (int fi = blockIdx.y; fi < nframes; fi += gridDim.y) {
        const int b = fi / nF, f = write_lo + (fi - b * nF);
        const int j = f - ramp_at;
        const bool ramp = prev != nullptr && j >= 0 && j < O;
        const float w = ramp ? rw[j] : 0.f;
        const int64_t vcs = (int64_t)Tw * hw, pcs = (int64_t)O * hw;           // channel strides of the window / the carry
        const bf16_t* vb = v + ((int64_t)b * 3 * Tw + f) * hw;
        const bf16_t* pb = ramp ? prev + ((int64_t)b * 3 * O + j) * hw : nullptr;
        uint8_t* ob = o + (int64_t)fi * hw * 3;
        if (VEC) {
            const int64_t G = hw >> 3;
            for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
                float c[3][8];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) unpack8(ld16_nt(vb + ch * vcs + g * 8), c[ch]);
                if (ramp) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        float a[8];
                        unpack8(ld16_nt(pb + ch * pcs + g * 8), a);
#pragma unroll
                        for (int k = 0; k < 8; ++k) c[ch][k] = window_blend(a[k], c[ch][k], w);
                    }
                }
                uint32_t word[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float px[3] = {c[0][k], c[1][k], c[2][k]};
                    uint8_t u[3];
                    postprocess_pixel(px, normalize, u);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) word[(3 * k + ch) >> 2] |= (uint32_t)u[ch] << (8 * ((3 * k + ch) & 3));
                }
                uint2* dst = reinterpret_cast<uint2*>(ob + g * 24);
                dst[0] = make_uint2(word[0], word[1]);
                dst[1] = make_uint2(word[2], word[3]);
                dst[2] = make_uint2(word[4], word[5]);
            }
        } else {
            for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (int64_t)gridDim.x * 256) {
                float c[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    c[ch] = bf2f(vb[ch * vcs + p]);
                    if (ramp) c[ch] = window_blend(bf2f(pb[ch * pcs + p]), c[ch], w);
                }
                uint8_t u[3];
                postprocess_pixel(c, normalize, u);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) ob[p * 3 + ch] = u[ch];
            }
        }
    }
}

// The one launch of the post-process: the whole-clip entry point is a window with no carry that writes every frame.
static int launch_postprocess(const void* video, const void* prev_tail, const void* ramp_w, void* out_u8, int B, int Tw, int H, int W,
                              int O, int ramp_at, int write_lo, int write_hi, int normalize_normal, void* stream) {
    const int nF = write_hi - write_lo;
    const int64_t hw = (int64_t)H * W, nframes = (int64_t)B * nF;
    DRN_CHECK_ARG(nframes < (1ll << 31));
    const bool vec = hw % 8 == 0 && ((uintptr_t)video & 15) == 0 && ((uintptr_t)prev_tail & 15) == 0 && ((uintptr_t)out_u8 & 7) == 0;
    const int64_t per_frame = vec ? hw / 8 : hw;
    int64_t gx = (per_frame + 255) / 256;
    if (gx > 4096) gx = 4096;
    const dim3 grid((unsigned)gx, (unsigned)(nframes < 65535 ? nframes : 65535));
    if (vec)
        postprocess_window_kernel<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
            (const bf16_t*)video, (const bf16_t*)prev_tail, (const float*)ramp_w, (uint8_t*)out_u8, (int)nframes, nF, Tw, hw, O,
            ramp_at, write_lo, normalize_normal);
    else
        postprocess_window_kernel<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
            (const bf16_t*)video, (const bf16_t*)prev_tail, (const float*)ramp_w, (uint8_t*)out_u8, (int)nframes, nF, Tw, hw, O,
            ramp_at, write_lo, normalize_normal);
    return drn_launch_status();
}

extern "C" int drn_postprocess_window_u8(const void* video, const void* prev_tail, const void* ramp_w, void* out_u8, int B, int Tw,
                                         int H, int W, int O, int ramp_at, int write_lo, int write_hi, int normalize_normal,
                                         void* stream) {
    DRN_CHECK_ARG(video && out_u8 && B > 0 && Tw > 0 && H > 0 && W > 0);
    DRN_CHECK_ARG((prev_tail == nullptr) == (ramp_w == nullptr));
    DRN_CHECK_ARG(O >= 0 && ramp_at >= 0 && (int64_t)ramp_at + O <= Tw);
    DRN_CHECK_ARG(0 <= write_lo && write_lo < write_hi && write_hi <= Tw);
    // a ramp is written whole or not at all: the frames in front of write_lo have no other writer
    if (prev_tail && O > 0) DRN_CHECK_ARG(write_lo <= ramp_at || write_lo >= ramp_at + O);
    DRN_CHECK_ARG(((uintptr_t)video & 1) == 0 && ((uintptr_t)prev_tail & 1) == 0 && ((uintptr_t)ramp_w & 3) == 0);
    return launch_postprocess(video, prev_tail, ramp_w, out_u8, B, Tw, H, W, O, ramp_at, write_lo, write_hi, normalize_normal, stream);
}

extern "C" int drn_postprocess_u8(const void* video, void* out_u8, int B, int T, int H, int W, int normalize_normal,
                                  void* stream) {
    DRN_CHECK_ARG(video && out_u8 && B > 0 && T > 0 && H > 0 && W > 0);
    return launch_postprocess(video, nullptr, nullptr, out_u8, B, T, H, W, 0, 0, 0, T, normalize_normal, stream);
}

extern "C" int drn_abi_version(void) { return DRN_ABI_VERSION; }

extern "C" const char* drn_error_string(int code) {
    if (code == DRN_OK) return "ok";
    if (code == DRN_EINVAL) return "drn: unsupported shape, stride or alignment (nothing launched)";
    return hipGetErrorString((hipError_t)code);
}
