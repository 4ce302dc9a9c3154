// Seed ensembles reduced per pixel (drn_ensemble_reduce_u8, include/drn.h; the torch specification: ensemble.py, reduce_members;
// DESIGN.md 4m).  N uint8 results of one shape, rendered under N seeds, become one: per byte the median or the mean of the N
// members, or, for normal maps, per pixel the renormalised vector sum; optionally with the members' spread around the result (the
// median / mean absolute deviation, or one minus the mean resultant length).  The members are N separate device buffers whose
// pointers travel BY VALUE in the kernel's argument struct: no stack of N tensors, no device table, no sort temporaries.
//
// Streaming, no scratch: per output byte N bytes in and one (with spread: two) out.  Where every base is 16-byte aligned a lane
// owns 16 bytes of every member (median, mean: one non-temporal 16-byte load per member, one 16-byte store per output) or 48
// bytes = 16 whole pixels (normal: three loads per member, three stores per output; a lane's piece never cuts a pixel).  Ragged
// bases go one byte (one pixel) per lane through the same arithmetic, which also finishes the vector path's tail.  The grid is
// capped and strided like elementwise.hip's ew_grid; offsets are 64-bit.
//
// median: the N unpacked bytes go through a compare-exchange network in registers (Batcher's odd-even merge sort for any N,
// generated at compile time as a constant pair list and fully unrolled; what the two middle outputs do not depend on is dropped
// by the compiler), r = the two middle values averaged half to even.  The spread sorts |m_k - r| through the same network: that
// second network exists only in the SPREAD instantiation.  mean: integer sum, divmod by the constant N, half to even.
// normal: fp32, every operation rounded on its own - plain operators under `fp contract(off)`, as in tile_blend.hip and
// sampler.hip and for the reason tile_blend.hip's header gives; no v_fma / v_pk_fma may stand in this file's arithmetic (the
// correctly rounded `/` and sqrtf expand to sequences that use them inside: that is the division, not a fusion).  A byte decodes
// through an LDS table of unit(i) * 2 - 1, unit(i) = fp32(i) / 255 correctly rounded (fit.hip's table, fit.u8_unit's bits).
#include "drn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EN_THREADS = 256;
constexpr int EN_MAX_BLOCKS = 2048;           // ew_grid's cap: one sweep of the 2048 * 256 lanes is 8 MiB (normal: 24 MiB)
constexpr int EN_MAX_N = 16;

struct EnMembers {
    const uint8_t* p[EN_MAX_N];
};

// ---------------------------------------------------------------------------------------------- the sorting network
struct EnNet {
    int n;
    unsigned char a[80], b[80];
};

// Batcher's odd-even merge sort in its iterative form, which sorts any n (63 exchanges at n = 16)
constexpr EnNet en_make_net(int n) {
    EnNet net = {};
    for (int p = 1; p < n; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < n; j += 2 * k)
                for (int i = 0; i < k && i + j + k < n; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        net.a[net.n] = (unsigned char)(i + j);
                        net.b[net.n] = (unsigned char)(i + j + k);
                        ++net.n;
                    }
    return net;
}

template <int N>
struct EnNetOf {
    static constexpr EnNet net = en_make_net(N);
};

// the two middle values of v[0..N) averaged, half to even (odd N: the middle value).  v is sorted in place.
template <int N>
__device__ __forceinline__ uint32_t en_median(uint32_t (&v)[N]) {
    constexpr EnNet net = EnNetOf<N>::net;
#pragma unroll
    for (int c = 0; c < net.n; ++c) {
        const uint32_t lo = min(v[net.a[c]], v[net.b[c]]), hi = max(v[net.a[c]], v[net.b[c]]);
        v[net.a[c]] = lo;
        v[net.b[c]] = hi;
    }
    const uint32_t t = v[(N - 1) / 2] + v[N / 2];
    uint32_t r = t >> 1;
    if (t & 1u) r += r & 1u;
    return r;
}

// the sum of v[0..N) over N, half to even
template <int N>
__device__ __forceinline__ uint32_t en_mean(const uint32_t (&v)[N]) {
    uint32_t S = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) S += v[k];
    const uint32_t q = S / (uint32_t)N, rem = S - q * (uint32_t)N;
    return q + ((2u * rem > (uint32_t)N || (2u * rem == (uint32_t)N && (q & 1u))) ? 1u : 0u);
}

// one byte position of the N members -> the result byte; sp = the same statistic of |m_k - r|
template <int N, int MODE, bool SPREAD>
__device__ __forceinline__ uint32_t en_byte(uint32_t (&v)[N], uint32_t& sp) {
    uint32_t d[N];
    if (SPREAD) {
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] = v[k];
    }
    const uint32_t r = MODE == 0 ? en_median<N>(v) : en_mean<N>(v);
    if (SPREAD) {
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] = d[k] > r ? d[k] - r : r - d[k];
        sp = MODE == 0 ? en_median<N>(d) : en_mean<N>(d);
    }
    return r;
}

// one pixel: s[] = the sum of the N decoded members in member order -> the result bytes o[], the spread byte
template <int N, bool SPREAD>
__device__ __forceinline__ void en_normal(const float (&s)[3], uint32_t (&o)[3], uint32_t& sp) {
    const float xx = s[0] * s[0], yy = s[1] * s[1], zz = s[2] * s[2];
    const float xy = xx + yy;
    const float l2 = xy + zz;
    const float l = sqrtf(l2);
    const float d = fmaxf(l, 1e-6f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float nc = s[c] / d;
        const float a = nc + 1.0f;
        const float m = a * 127.5f;
        o[c] = (uint32_t)__builtin_rintf(__builtin_amdgcn_fmed3f(m, 0.0f, 255.0f));
    }
    if (SPREAD) {
        const float q = l / (float)N;
        const float e = 1.0f - q;
        const float w = 255.0f * __builtin_amdgcn_fmed3f(e, 0.0f, 1.0f);
        sp = (uint32_t)__builtin_rintf(w);
    }
}

// MODE 0 median, 1 mean, 2 normal.  n: bytes.  vec: every base is 16-byte aligned (the host's finding; uniform).
template <int N, int MODE, bool SPREAD>
__global__ void __launch_bounds__(EN_THREADS) ensemble_reduce_kernel(EnMembers mem, uint8_t* __restrict__ dst,
                                                                     uint8_t* __restrict__ spread, int64_t n, int vec) {
    __shared__ float dec_s[256];                                  // MODE 2: byte -> unit(byte) * 2 - 1
    if (MODE == 2) {
        const float u = __fdiv_rn((float)threadIdx.x, 255.0f);
        const float u2 = u * 2.0f;
        dec_s[threadIdx.x] = u2 - 1.0f;
        __syncthreads();
    }
    const int64_t lane = (int64_t)blockIdx.x * EN_THREADS + threadIdx.x;
    const int64_t lanes = (int64_t)gridDim.x * EN_THREADS;
    if (MODE != 2) {
        const int64_t nv = vec ? n >> 4 : 0;
        for (int64_t g = lane; g < nv; g += lanes) {
            const int64_t e = g << 4;
            uint32_t w[N][4];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const uint4 q = ld16_nt(mem.p[k] + e);
                w[k][0] = q.x; w[k][1] = q.y; w[k][2] = q.z; w[k][3] = q.w;
            }
            uint32_t o[4], s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = 0;
                s[j] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    uint32_t v[N], sp = 0;
#pragma unroll
                    for (int k = 0; k < N; ++k) v[k] = (w[k][j] >> (8 * b)) & 255u;
                    o[j] |= en_byte<N, MODE, SPREAD>(v, sp) << (8 * b);
                    s[j] |= sp << (8 * b);
                }
            }
            *reinterpret_cast<uint4*>(dst + e) = make_uint4(o[0], o[1], o[2], o[3]);
            if (SPREAD) *reinterpret_cast<uint4*>(spread + e) = make_uint4(s[0], s[1], s[2], s[3]);
        }
        for (int64_t i = (nv << 4) + lane; i < n; i += lanes) {
            uint32_t v[N], sp = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = mem.p[k][i];
            dst[i] = (uint8_t)en_byte<N, MODE, SPREAD>(v, sp);
            if (SPREAD) spread[i] = (uint8_t)sp;
        }
    } else {
        const int64_t nv = vec ? n / 48 : 0;                      // pieces of 16 whole pixels
        for (int64_t g = lane; g < nv; g += lanes) {
            const int64_t e = g * 48;
            // 16 bytes of every member at a time (the sum is per byte; only the normalisation below needs whole pixels): a
            // round's N loads are issued together, then member after member is decoded and added.  The rounds and the members
            // are kept apart for the scheduler: left alone, hipcc hoists all 3 N loads and all 48 N table reads and runs out of
            // registers from N = 5 on
            float s[48];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                uint32_t w[N][4];
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const uint4 q = ld16_nt(mem.p[k] + e + 16 * j);
                    w[k][0] = q.x; w[k][1] = q.y; w[k][2] = q.z; w[k][3] = q.w;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < N; ++k) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float v = dec_s[(w[k][i >> 2] >> (8 * (i & 3))) & 255u];
                        s[16 * j + i] = k == 0 ? v : s[16 * j + i] + v;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            uint32_t ob[48], sb[48];
#pragma unroll
            for (int px = 0; px < 16; ++px) {
                const float sv[3] = {s[3 * px], s[3 * px + 1], s[3 * px + 2]};
                uint32_t o[3], sp = 0;
                en_normal<N, SPREAD>(sv, o, sp);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    ob[3 * px + c] = o[c];
                    sb[3 * px + c] = sp;
                }
                if ((px & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                uint32_t ow[4], sw[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int b = 16 * j + 4 * i;
                    ow[i] = ob[b] | (ob[b + 1] << 8) | (ob[b + 2] << 16) | (ob[b + 3] << 24);
                    sw[i] = sb[b] | (sb[b + 1] << 8) | (sb[b + 2] << 16) | (sb[b + 3] << 24);
                }
                *reinterpret_cast<uint4*>(dst + e + 16 * j) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
                if (SPREAD) *reinterpret_cast<uint4*>(spread + e + 16 * j) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
            }
        }
        const int64_t npx = n / 3;
        for (int64_t px = nv * 16 + lane; px < npx; px += lanes) {
            const int64_t i = px * 3;
            float s[3];
#pragma unroll
            for (int k = 0; k < N; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = dec_s[mem.p[k][i + c]];
                    s[c] = k == 0 ? v : s[c] + v;
                }
            }
            uint32_t o[3], sp = 0;
            en_normal<N, SPREAD>(s, o, sp);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dst[i + c] = (uint8_t)o[c];
                if (SPREAD) spread[i + c] = (uint8_t)sp;
            }
        }
    }
}

template <int N>
void en_launch(int mode, dim3 grid, hipStream_t stream, const EnMembers& mem, uint8_t* dst, uint8_t* spread, int64_t n, int vec) {
    const dim3 block(EN_THREADS);
    if (spread) {
        if (mode == 0) ensemble_reduce_kernel<N, 0, true><<<grid, block, 0, stream>>>(mem, dst, spread, n, vec);
        else if (mode == 1) ensemble_reduce_kernel<N, 1, true><<<grid, block, 0, stream>>>(mem, dst, spread, n, vec);
        else ensemble_reduce_kernel<N, 2, true><<<grid, block, 0, stream>>>(mem, dst, spread, n, vec);
    } else {
        if (mode == 0) ensemble_reduce_kernel<N, 0, false><<<grid, block, 0, stream>>>(mem, dst, nullptr, n, vec);
        else if (mode == 1) ensemble_reduce_kernel<N, 1, false><<<grid, block, 0, stream>>>(mem, dst, nullptr, n, vec);
        else ensemble_reduce_kernel<N, 2, false><<<grid, block, 0, stream>>>(mem, dst, nullptr, n, vec);
    }
}

// ---------------------------------------------------------------------------------------------- the reduce behind an affine
// Ensembles that agree (ensemble.py; the solve: ensemble_align.hip): member k's byte x of clip b is read as
// u8(rint(clamp(fp32(g * fp32(x)) + o, 0, 255))) with (g, o) = affine[k][b] - torch's m.float() * g + o, two separately rounded
// operations under this file's `fp contract(off)`, then the clamp, then half to even - and the median / mean and the spread are
// the rules above on those bytes.  (1, 0) gives the byte back.  blockIdx.y strides the clips, so the 2 N values of a clip's
// affines are uniform and a lane's 16 bytes never cross from one clip into the next: the wide path needs every clip's base on
// the 16-byte grid (the host's finding, `vec`).
__device__ __forceinline__ uint32_t en_affine(uint32_t x, float g, float o) {
    const float m = g * (float)x;
    const float a = m + o;
    return (uint32_t)__builtin_rintf(__builtin_amdgcn_fmed3f(a, 0.0f, 255.0f));
}

template <int N, int MODE, bool SPREAD>
__global__ void __launch_bounds__(EN_THREADS) ensemble_reduce_affine_kernel(EnMembers mem, const float* __restrict__ affine, int B,
                                                                            int64_t clip_bytes, uint8_t* __restrict__ dst,
                                                                            uint8_t* __restrict__ spread, int vec) {
    const int64_t lane = (int64_t)blockIdx.x * EN_THREADS + threadIdx.x;
    const int64_t lanes = (int64_t)gridDim.x * EN_THREADS;
    const int64_t n = clip_bytes;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        float ag[N], ao[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            ag[k] = affine[((int64_t)k * B + b) * 2];
            ao[k] = affine[((int64_t)k * B + b) * 2 + 1];
        }
        const int64_t base = (int64_t)b * n;
        const int64_t nv = vec ? n >> 4 : 0;
        for (int64_t g = lane; g < nv; g += lanes) {
            const int64_t e = base + (g << 4);
            uint32_t w[N][4];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const uint4 q = ld16_nt(mem.p[k] + e);
                w[k][0] = q.x; w[k][1] = q.y; w[k][2] = q.z; w[k][3] = q.w;
            }
            uint32_t o[4], s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = 0;
                s[j] = 0;
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    uint32_t v[N], sp = 0;
#pragma unroll
                    for (int k = 0; k < N; ++k) v[k] = en_affine((w[k][j] >> (8 * bb)) & 255u, ag[k], ao[k]);
                    o[j] |= en_byte<N, MODE, SPREAD>(v, sp) << (8 * bb);
                    s[j] |= sp << (8 * bb);
                }
            }
            *reinterpret_cast<uint4*>(dst + e) = make_uint4(o[0], o[1], o[2], o[3]);
            if (SPREAD) *reinterpret_cast<uint4*>(spread + e) = make_uint4(s[0], s[1], s[2], s[3]);
        }
        for (int64_t i = (nv << 4) + lane; i < n; i += lanes) {
            uint32_t v[N], sp = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = en_affine(mem.p[k][base + i], ag[k], ao[k]);
            dst[base + i] = (uint8_t)en_byte<N, MODE, SPREAD>(v, sp);
            if (SPREAD) spread[base + i] = (uint8_t)sp;
        }
    }
}

template <int N>
void en_launch_affine(int mode, dim3 grid, hipStream_t stream, const EnMembers& mem, const float* affine, int B, int64_t clip_bytes,
                      uint8_t* dst, uint8_t* spread, int vec) {
    const dim3 block(EN_THREADS);
    if (spread) {
        if (mode == 0) ensemble_reduce_affine_kernel<N, 0, true><<<grid, block, 0, stream>>>(mem, affine, B, clip_bytes, dst, spread, vec);
        else ensemble_reduce_affine_kernel<N, 1, true><<<grid, block, 0, stream>>>(mem, affine, B, clip_bytes, dst, spread, vec);
    } else {
        if (mode == 0) ensemble_reduce_affine_kernel<N, 0, false><<<grid, block, 0, stream>>>(mem, affine, B, clip_bytes, dst, nullptr, vec);
        else ensemble_reduce_affine_kernel<N, 1, false><<<grid, block, 0, stream>>>(mem, affine, B, clip_bytes, dst, nullptr, vec);
    }
}

}  // namespace

extern "C" int drn_ensemble_reduce_u8(const void* const* members, int N, void* dst, void* spread, int64_t n_bytes, int mode,
                                      void* stream) {
    DRN_CHECK_ARG(members && dst);
    DRN_CHECK_ARG(N >= 1 && N <= EN_MAX_N);
    DRN_CHECK_ARG(mode >= 0 && mode <= 2);
    DRN_CHECK_ARG(n_bytes >= 0);
    DRN_CHECK_ARG(mode != 2 || n_bytes % 3 == 0);
    DRN_CHECK_ARG(dst != spread);
    EnMembers mem = {};
    uintptr_t all = (uintptr_t)dst | (uintptr_t)spread;
    for (int k = 0; k < N; ++k) {
        DRN_CHECK_ARG(members[k] && members[k] != dst && members[k] != spread);
        mem.p[k] = (const uint8_t*)members[k];
        all |= (uintptr_t)members[k];
    }
    if (n_bytes == 0) return DRN_OK;
    const int vec = (all & 15) == 0;
    // lanes wanted: the vector path's pieces (and, far fewer, the tail's bytes or pixels), or every byte / pixel
    const int64_t piece = mode == 2 ? 48 : 16, unit = mode == 2 ? 3 : 1;
    const int64_t pieces = n_bytes / piece, tail = (n_bytes - pieces * piece) / unit;
    const int64_t work = vec ? (pieces > tail ? pieces : tail) : n_bytes / unit;
    int64_t blocks = (work + EN_THREADS - 1) / EN_THREADS;
    if (blocks > EN_MAX_BLOCKS) blocks = EN_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *pd = (uint8_t*)dst, *ps = (uint8_t*)spread;
    switch (N) {
#define EN_CASE(n_) case n_: en_launch<n_>(mode, grid, st, mem, pd, ps, n_bytes, vec); break;
        EN_CASE(1) EN_CASE(2) EN_CASE(3) EN_CASE(4) EN_CASE(5) EN_CASE(6) EN_CASE(7) EN_CASE(8)
        EN_CASE(9) EN_CASE(10) EN_CASE(11) EN_CASE(12) EN_CASE(13) EN_CASE(14) EN_CASE(15) EN_CASE(16)
#undef EN_CASE
    }
    return drn_launch_status();
}

extern "C" int drn_ensemble_reduce_affine_u8(const void* const* members, int N, const void* affine, int B, int64_t clip_bytes,
                                             void* dst, void* spread, int mode, void* stream) {
    DRN_CHECK_ARG(mode >= 0 && mode <= 1);
    DRN_CHECK_ARG(B >= 1 && clip_bytes >= 0 && clip_bytes <= INT64_MAX / B);
    DRN_CHECK_ARG(((uintptr_t)affine & 3) == 0);
    if (!affine) return drn_ensemble_reduce_u8(members, N, dst, spread, (int64_t)B * clip_bytes, mode, stream);
    DRN_CHECK_ARG(members && dst);
    DRN_CHECK_ARG(N >= 1 && N <= EN_MAX_N);
    DRN_CHECK_ARG(dst != spread);
    EnMembers mem = {};
    uintptr_t all = (uintptr_t)dst | (uintptr_t)spread;
    for (int k = 0; k < N; ++k) {
        DRN_CHECK_ARG(members[k] && members[k] != dst && members[k] != spread);
        mem.p[k] = (const uint8_t*)members[k];
        all |= (uintptr_t)members[k];
    }
    if (clip_bytes == 0) return DRN_OK;
    if (B > 1) all |= (uintptr_t)clip_bytes;                          // every clip's base on the 16-byte grid, or one byte per lane
    const int vec = (all & 15) == 0;
    const int64_t pieces = clip_bytes / 16, tail = clip_bytes - pieces * 16;
    const int64_t work = vec ? (pieces > tail ? pieces : tail) : clip_bytes;
    int64_t blocks = (work + EN_THREADS - 1) / EN_THREADS;
    if (blocks > EN_MAX_BLOCKS) blocks = EN_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks, (unsigned)(B < 65535 ? B : 65535));
    hipStream_t st = (hipStream_t)stream;
    switch (N) {
#define EN_CASE(n_) \
    case n_: en_launch_affine<n_>(mode, grid, st, mem, (const float*)affine, B, clip_bytes, (uint8_t*)dst, (uint8_t*)spread, vec); break;
        EN_CASE(1) EN_CASE(2) EN_CASE(3) EN_CASE(4) EN_CASE(5) EN_CASE(6) EN_CASE(7) EN_CASE(8)
        EN_CASE(9) EN_CASE(10) EN_CASE(11) EN_CASE(12) EN_CASE(13) EN_CASE(14) EN_CASE(15) EN_CASE(16)
#undef EN_CASE
    }
    return drn_launch_status();
}
