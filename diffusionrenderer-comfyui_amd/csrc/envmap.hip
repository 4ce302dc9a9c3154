// Environment-light projection of the forward renderer under a per-frame y-rotation (drn_env_project, include/drn.h):
// every frame's lat-long directions rotated, looked up in the cube map and tone-mapped, in ONE launch over T*H*W pixels.
// Restates preprocess_envmap.py's torch path (rotate -> negate -> cube_lookup -> flip -> hdr_mapping_official -> *2-1) op for
// op, in the order of the torch ops, so the result stays within a few ulp of it: accurate powf / log1pf / division only, no
// fast-math flags, no contraction of a multiply and an add that torch rounds separately.
//
// A light that changes over the clip (an env-map sequence, one panorama per frame) adds two entries: drn_env_cubes builds the
// cube maps of a run of panoramas in one launch (latlong_to_cubemap_official's grid_sample on apply_hdr_preprocessing's
// clean-up, from a sampling grid the host computed), and drn_env_project_seq is the projection with every frame's cube map
// taken from a table - the same kernel as drn_env_project, which passes no table.
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

// cube_of: NULL = every frame looks up cube map 0 (drn_env_project), else frame t looks up cube map cube_of[t], clamped into
// [0, n_cubes).  Frame t is stored at frame t0 + t of outputs that hold T_all frames.
__global__ void __launch_bounds__(256) env_project_kernel(const float* __restrict__ cube, int n_cubes,
                                                          const int* __restrict__ cube_of, int R, const float* __restrict__ vec,
                                                          const float* __restrict__ rot, float* __restrict__ env_ldr,
                                                          float* __restrict__ env_log, int T, int t0, int T_all, int H, int W,
                                                          float log_den) {
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
    const int k = cube_of ? min(max(cube_of[t], 0), n_cubes - 1) : 0;
    const float* f = cube + ((int64_t)k * 6 + face) * R * R * 3;
    const float* p_nw = f + ((int64_t)y0 * R + x0) * 3;
    const float* p_ne = f + ((int64_t)y0 * R + x1) * 3;
    const float* p_sw = f + ((int64_t)y1 * R + x0) * 3;
    const float* p_se = f + ((int64_t)y1 * R + x1) * 3;

    // the two flips: pixel (h, w) of the projection lands at (H-1-h, W-1-w); lanes walk w, so stores stay contiguous
    const int64_t plane = (int64_t)T_all * H * W;
    const int64_t o = ((int64_t)(t0 + t) * H + (H - 1 - h)) * W + (W - 1 - w);
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

// texel_coord with the product and the subtraction in ONE fused multiply-add.  latlong_to_cubemap_official is torch's grid_sample,
// and torch's builds (CPU and device alike) contract `(g + 1) * size - 1` of its unnormalisation: with the two roundings of
// texel_coord a quarter of the cube texels land one ulp of a coordinate (3.8e-6 near column 47) beside torch's, which times the
// step between neighbouring HDR texels is 1e-4 in the cube map and, through env_ldr's slope of ~400 near 0, 2e-3 in the
// conditions.  The cube lookup of the projection above keeps texel_coord: there it is pinned by drn_env_project's tests.
__device__ __forceinline__ float texel_coord_fused(float g, int size) {
    const float u = fmaf(g + 1.0f, (float)size, -1.0f) / 2.0f;
    return fminf((float)(size - 1), fmaxf(u, 0.0f));
}

// apply_hdr_preprocessing's clean-up of one panorama value: `* brightness` only when it is not 1.0, then
// nan_to_num(nan=0, posinf=65504, neginf=0), then clamp(0, 65504)
__device__ __forceinline__ float clean_tap(float v, float brightness, bool scale) {
    if (scale) v = v * brightness;
    if (v != v) v = 0.0f;
    return fminf(fmaxf(v, 0.0f), 65504.0f);          // +inf -> 65504 and -inf -> 0 are what the clamp gives them
}

// One thread per cube texel of one panorama.  The source column of cleaned-panorama column c: the flip comes before the roll,
// rolled[c] = flipped[(c - roll) mod We], flipped[j] = raw[We - 1 - j].
__global__ void __launch_bounds__(256) env_cubes_kernel(const float* __restrict__ latlong, const float* __restrict__ grid,
                                                        float* __restrict__ cubes, int He, int We, int R, int n0, int n,
                                                        float brightness, int flip, int roll) {
    const int64_t per = (int64_t)6 * R * R;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * n) return;
    const int k = (int)(idx / per);
    const int64_t texel = idx - (int64_t)k * per;
    const float gx = grid[2 * texel], gy = grid[2 * texel + 1];

    const float ix = texel_coord_fused(gx, We), iy = texel_coord_fused(gy, He);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const bool x1_in = x0 + 1 <= We - 1, y1_in = y0 + 1 <= He - 1;
    const int x1 = x1_in ? x0 + 1 : x0, y1 = y1_in ? y0 + 1 : y0;
    const float wx1 = ix - x0f, wx0 = (x0f + 1.0f) - ix, wy1 = iy - y0f, wy0 = (y0f + 1.0f) - iy;
    const float w_nw = wx0 * wy0, w_ne = wx1 * wy0, w_sw = wx0 * wy1, w_se = wx1 * wy1;

    int c0 = x0 - roll, c1 = x1 - roll;
    c0 = c0 < 0 ? c0 + We : c0;
    c1 = c1 < 0 ? c1 + We : c1;
    if (flip) {
        c0 = We - 1 - c0;
        c1 = We - 1 - c1;
    }
    const float* src = latlong + (int64_t)(n0 + k) * He * We * 3;
    const float* p_nw = src + ((int64_t)y0 * We + c0) * 3;
    const float* p_ne = src + ((int64_t)y0 * We + c1) * 3;
    const float* p_sw = src + ((int64_t)y1 * We + c0) * 3;
    const float* p_se = src + ((int64_t)y1 * We + c1) * 3;
    const bool scale = brightness != 1.0f;
    float* o = cubes + idx * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float e = clean_tap(p_nw[ch], brightness, scale) * w_nw;
        e += (x1_in ? clean_tap(p_ne[ch], brightness, scale) : 0.0f) * w_ne;
        e += (y1_in ? clean_tap(p_sw[ch], brightness, scale) : 0.0f) * w_sw;
        e += (x1_in && y1_in ? clean_tap(p_se[ch], brightness, scale) : 0.0f) * w_se;
        o[ch] = e;
    }
}

int env_project_launch(const float* cube, int n_cubes, const int* cube_of, int R, const float* vec, const float* rot,
                       float* env_ldr, float* env_log, int T, int t0, int T_all, int H, int W, float log_scale, void* stream) {
    DRN_CHECK_ARG(cube && vec && rot && env_ldr && env_log);
    DRN_CHECK_ARG(R >= 1 && T >= 1 && H >= 1 && W >= 1);
    DRN_CHECK_ARG(n_cubes >= 1 && t0 >= 0 && (int64_t)t0 + T <= T_all);
    const int64_t n = (int64_t)T * H * W;
    DRN_CHECK_ARG((int64_t)T_all * H * W < ((int64_t)1 << 31));
    DRN_CHECK_ARG((((uintptr_t)cube | (uintptr_t)vec | (uintptr_t)rot | (uintptr_t)env_ldr | (uintptr_t)env_log |
                    (uintptr_t)cube_of) & 3) == 0);
    const float log_den = (float)log1p((double)log_scale);          // np.log1p(log_scale), rounded where torch rounds it
    env_project_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        cube, n_cubes, cube_of, R, vec, rot, env_ldr, env_log, T, t0, T_all, H, W, log_den);
    return drn_launch_status();
}

}  // namespace

extern "C" int drn_env_cubes(const float* latlong, const float* grid, float* cubes, int N, int He, int We, int R, int n0, int n,
                             float brightness, int flip, int roll, void* stream) {
    DRN_CHECK_ARG(latlong && grid && cubes);
    DRN_CHECK_ARG(N >= 1 && He >= 1 && We >= 1 && R >= 1);
    DRN_CHECK_ARG(n0 >= 0 && n >= 1 && (int64_t)n0 + n <= N);
    DRN_CHECK_ARG(roll >= 0 && roll < We);
    DRN_CHECK_ARG((((uintptr_t)latlong | (uintptr_t)grid | (uintptr_t)cubes) & 3) == 0);
    const int64_t texels = (int64_t)n * 6 * R * R;
    DRN_CHECK_ARG((int64_t)N * He * We * 3 < ((int64_t)1 << 31) && texels * 3 < ((int64_t)1 << 31));
    env_cubes_kernel<<<dim3((unsigned)((texels + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        latlong, grid, cubes, He, We, R, n0, n, brightness, flip, roll);
    return drn_launch_status();
}

extern "C" int drn_env_project_seq(const float* cubes, int n_cubes, const int32_t* cube_of, int R, const float* vec,
                                   const float* rot, float* env_ldr, float* env_log, int T, int t0, int T_all, int H, int W,
                                   float log_scale, void* stream) {
    DRN_CHECK_ARG(cube_of);
    return env_project_launch(cubes, n_cubes, cube_of, R, vec, rot, env_ldr, env_log, T, t0, T_all, H, W, log_scale, stream);
}

extern "C" int drn_env_project(const float* cube, int R, const float* vec, const float* rot, float* env_ldr, float* env_log,
                               int T, int H, int W, float log_scale, void* stream) {
    return env_project_launch(cube, 1, nullptr, R, vec, rot, env_ldr, env_log, T, 0, T, H, W, log_scale, stream);
}
