// Environment-light projection of the forward renderer under a per-frame y-rotation (drn_env_project, include/drn.h):
// every frame's lat-long directions rotated, looked up in the cube map and tone-mapped, in ONE launch over T*H*W pixels.
// Restates preprocess_envmap.py's torch path (rotate -> negate -> cube_lookup -> flip -> hdr_mapping_official -> *2-1) op for
// op, in the order of the torch ops, so the result stays within a few ulp of it: accurate powf / log1pf / division only, no
// fast-math flags, no contraction of a multiply and an add that torch rounds separately.
#include "drn_common.h"

#pragma clang fp contract(off)

namespace {

// rgb2srgb_official: where(rgb <= 0.0031308, 12.92 rgb, 1.055 pow(clamp(rgb, 1e-8, 1), 1/2.4) - 0.055)
__device__ __forceinline__ float srgb(float v) {
    const float p = 1.055f * powf(fminf(fmaxf(v, 1e-8f), 1.0f), (float)(1.0 / 2.4)) - 0.055f;
    return v <= 0.0031308f ? 12.92f * v : p;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// grid_sample's align_corners=False unnormalisation + border clamp of one coordinate (face coordinate in [-1, 1] -> texel units)
__device__ __forceinline__ float texel_coord(float g, int R) {
    const float u = ((g + 1.0f) * (float)R - 1.0f) / 2.0f;
    return fminf((float)(R - 1), fmaxf(u, 0.0f));
}

__global__ void __launch_bounds__(256) env_project_kernel(const float* __restrict__ cube, int R, const float* __restrict__ vec,
                                                          const float* __restrict__ rot, float* __restrict__ env_ldr,
                                                          float* __restrict__ env_log, int T, int H, int W, float log_den) {
    const int64_t n = (int64_t)T * H * W;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int w = (int)(idx % W);
    const int h = (int)((idx / W) % H);
    const int t = (int)(idx / ((int64_t)W * H));

    // vec @ rotate_y(theta_t)[:3, :3].T, then the negation of the query
    const float* v = vec + ((int64_t)h * W + w) * 3;
    const float vx = v[0], vy = v[1], vz = v[2];
    const float c = rot[2 * t], s = rot[2 * t + 1];
    const float x = -(c * vx + s * vz);
    const float y = -vy;
    const float z = -(c * vz - s * vx);

    // cube_lookup: major-axis face with its comparisons, face coordinates divided by the major axis
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const bool is_x = ax >= ay && ax >= az;
    const bool is_y = !is_x && ay >= az;
    const float ma = fmaxf(is_x ? ax : (is_y ? ay : az), 1e-12f);
    const int face = is_x ? (x > 0.0f ? 0 : 1) : (is_y ? (y > 0.0f ? 2 : 3) : (z > 0.0f ? 4 : 5));
    const float fx = (is_x ? (x > 0.0f ? -z : z) : (is_y ? x : (z > 0.0f ? x : -x))) / ma;
    const float fy = (is_x ? -y : (is_y ? (y > 0.0f ? z : -z) : -y)) / ma;

    // per-face bilinear fetch, grid_sample(mode="bilinear", padding_mode="border", align_corners=False)
    const float ix = texel_coord(fx, R), iy = texel_coord(fy, R);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const bool x1_in = x0 + 1 <= R - 1, y1_in = y0 + 1 <= R - 1;        // the clamped coordinate never leaves on the low side
    const int x1 = x1_in ? x0 + 1 : x0, y1 = y1_in ? y0 + 1 : y0;
    const float wx1 = ix - x0f, wx0 = (x0f + 1.0f) - ix, wy1 = iy - y0f, wy0 = (y0f + 1.0f) - iy;
    const float w_nw = wx0 * wy0, w_ne = wx1 * wy0, w_sw = wx0 * wy1, w_se = wx1 * wy1;
    const float* f = cube + (int64_t)face * R * R * 3;
    const float* p_nw = f + ((int64_t)y0 * R + x0) * 3;
    const float* p_ne = f + ((int64_t)y0 * R + x1) * 3;
    const float* p_sw = f + ((int64_t)y1 * R + x0) * 3;
    const float* p_se = f + ((int64_t)y1 * R + x1) * 3;

    // the two flips: pixel (h, w) of the projection lands at (H-1-h, W-1-w); lanes walk w, so stores stay contiguous
    const int64_t plane = (int64_t)T * H * W;
    const int64_t o = ((int64_t)t * H + (H - 1 - h)) * W + (W - 1 - w);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float e = p_nw[ch] * w_nw;
        e += (x1_in ? p_ne[ch] : 0.0f) * w_ne;
        e += (y1_in ? p_sw[ch] : 0.0f) * w_sw;
        e += (x1_in && y1_in ? p_se[ch] : 0.0f) * w_se;
        // hdr_mapping_official: env_ev0 = srgb(clamp(reinhard(e, 16), 0, 1)); env_log = clamp(srgb(log1p(e) / log1p(log_scale)), 0, 1)
        const float ev0 = srgb(clamp01(e / (e + 1.0f) * 16.0f));
        const float lg = clamp01(srgb(log1pf(e) / log_den));
        env_ldr[ch * plane + o] = ev0 * 2.0f - 1.0f;
        env_log[ch * plane + o] = lg * 2.0f - 1.0f;
    }
}

}  // namespace

extern "C" int drn_env_project(const float* cube, int R, const float* vec, const float* rot, float* env_ldr, float* env_log,
                               int T, int H, int W, float log_scale, void* stream) {
    DRN_CHECK_ARG(cube && vec && rot && env_ldr && env_log);
    DRN_CHECK_ARG(R >= 1 && T >= 1 && H >= 1 && W >= 1);
    const int64_t n = (int64_t)T * H * W;
    DRN_CHECK_ARG(n < ((int64_t)1 << 31));
    DRN_CHECK_ARG((((uintptr_t)cube | (uintptr_t)vec | (uintptr_t)rot | (uintptr_t)env_ldr | (uintptr_t)env_log) & 3) == 0);
    const float log_den = (float)log1p((double)log_scale);          // np.log1p(log_scale), rounded where torch rounds it
    env_project_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        cube, R, vec, rot, env_ldr, env_log, T, H, W, log_den);
    return drn_launch_status();
}
