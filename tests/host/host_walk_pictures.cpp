// host walk, the picture family: uint8 post-process and windows, environment light, fit / restore / guided restore, spatial and
// latent tiles, seed ensembles.  Sections A and D of the walk for these entries.
#include "host_walk.h"

namespace hw {
namespace {

const int64_t G = 1ll << 30;

// ---- drn_postprocess_u8
struct Pp { bool v = 1, o = 1; int B = 2, T = 5, H = 48, W = 40, norm = 1; int v_mis = 0; };
int pp(const Pp& p) {
    const int64_t px = (int64_t)p.B * p.T * p.H * p.W * 3;
    return drn_postprocess_u8(p.v ? A("video", px * 2, p.v_mis) : 0, p.o ? A("out_u8", px) : 0, p.B, p.T, p.H, p.W, p.norm, STREAM);
}

// ---- drn_postprocess_window_u8 / drn_postprocess_window_align_u8
struct Pw { bool v = 1, prev = 1, rw = 1, o = 1, aff = 1, carry = 1; int carry_is = 0;   // 1: carry_out == prev_tail, 2: == video
            int B = 2, Tw = 9, H = 48, W = 40, O = 3, ramp_at = 0, lo = 0, hi = 9, norm = 0; int v_mis = 0, prev_mis = 0, rw_mis = 0, aff_mis = 0, carry_mis = 0; };
int pw(const Pw& p) {
    const int64_t hw = (int64_t)p.H * p.W;
    return drn_postprocess_window_u8(p.v ? A("video", p.B * 3 * p.Tw * hw * 2, p.v_mis) : 0, p.prev ? A("prev_tail", p.B * 3 * p.O * hw * 2, p.prev_mis) : 0,
                                     p.rw ? A("ramp_w", p.O * 4, p.rw_mis) : 0, p.o ? A("out_u8", (int64_t)p.B * (p.hi - p.lo) * hw * 3) : 0, p.B,
                                     p.Tw, p.H, p.W, p.O, p.ramp_at, p.lo, p.hi, p.norm, STREAM);
}
int pwa(const Pw& p) {
    const int64_t hw = (int64_t)p.H * p.W;
    void* v = p.v ? A("video", p.B * 3 * p.Tw * hw * 2, p.v_mis) : 0;
    void* prev = p.prev ? A("prev_tail", p.B * 3 * p.O * hw * 2, p.prev_mis) : 0;
    void* carry = p.carry_is == 1 ? prev : p.carry_is == 2 ? v : (p.carry ? A("carry_out", p.B * 3 * p.O * hw * 2, p.carry_mis) : 0);
    return drn_postprocess_window_align_u8(v, prev, p.rw ? A("ramp_w", p.O * 4, p.rw_mis) : 0, p.aff ? A("affine", p.B * 8, p.aff_mis) : 0,
                                           p.o ? A("out_u8", (int64_t)p.B * (p.hi - p.lo) * hw * 3) : 0, carry, p.B, p.Tw, p.H, p.W, p.O,
                                           p.ramp_at, p.lo, p.hi, p.norm, STREAM);
}

// ---- drn_window_align_affine
struct Wa { bool v = 1, prev = 1, aff = 1, mom = 1, ws = 1; int B = 2, Tw = 9, H = 48, W = 40, O = 3, ramp_at = 0; int64_t ws_short = 0;
            int v_mis = 0, aff_mis = 0, mom_mis = 0, ws_mis = 0; };
int wa(const Wa& p) {
    const int64_t hw = (int64_t)p.H * p.W, need = drn_window_align_workspace_bytes(p.B, p.H, p.W, p.O) - p.ws_short;
    return drn_window_align_affine(p.v ? A("video", p.B * 3 * p.Tw * hw * 2, p.v_mis) : 0, p.prev ? A("prev_tail", p.B * 3 * p.O * hw * 2) : 0,
                                   p.aff ? A("affine", p.B * 8, p.aff_mis) : 0, p.mom ? A("moments", p.B * 48, p.mom_mis) : 0,
                                   p.ws ? A("workspace", need, p.ws_mis) : 0, need, p.B, p.Tw, p.H, p.W, p.O, p.ramp_at, STREAM);
}

// ---- environment light
struct Ev { bool cube = 1, vec = 1, rot = 1, ldr = 1, log = 1, cof = 1; int R = 64, T = 5, H = 32, W = 64, n_cubes = 3, t0 = 1, T_all = 7; int mis = 0, cof_mis = 0; };
int ev(const Ev& p) {
    const int64_t out = 3ll * p.T * p.H * p.W * 4;
    return drn_env_project(p.cube ? (float*)A("cube", 6ll * p.R * p.R * 12, p.mis) : 0, p.R, p.vec ? (float*)A("vec", (int64_t)p.H * p.W * 12) : 0,
                           p.rot ? (float*)A("rot", p.T * 8) : 0, p.ldr ? (float*)A("env_ldr", out) : 0, p.log ? (float*)A("env_log", out) : 0,
                           p.T, p.H, p.W, 10000.f, STREAM);
}
int evs(const Ev& p) {
    const int64_t out = 3ll * p.T_all * p.H * p.W * 4;
    return drn_env_project_seq(p.cube ? (float*)A("cubes", 6ll * p.n_cubes * p.R * p.R * 12, p.mis) : 0, p.n_cubes,
                               p.cof ? (int32_t*)A("cube_of", p.T * 4, p.cof_mis) : 0, p.R, p.vec ? (float*)A("vec", (int64_t)p.H * p.W * 12) : 0,
                               p.rot ? (float*)A("rot", p.T * 8) : 0, p.ldr ? (float*)A("env_ldr", out) : 0, p.log ? (float*)A("env_log", out) : 0,
                               p.T, p.t0, p.T_all, p.H, p.W, 10000.f, STREAM);
}
struct Ec { bool ll = 1, grid = 1, cubes = 1; int N = 4, He = 64, We = 128, R = 32, n0 = 1, n = 2, roll = 5; int mis = 0; };
int ec(const Ec& p) {
    return drn_env_cubes(p.ll ? (float*)A("latlong", (int64_t)p.N * p.He * p.We * 12, p.mis) : 0, p.grid ? (float*)A("grid", 6ll * p.R * p.R * 8) : 0,
                         p.cubes ? (float*)A("cubes", 6ll * p.n * p.R * p.R * 12) : 0, p.N, p.He, p.We, p.R, p.n0, p.n, 1.5f, 1, p.roll, STREAM);
}

// ---- fit, restore, guided restore
struct Ft { bool src = 1, dst = 1, tidx = 1, ylo = 1, yw = 1, xlo = 1, xw = 1, gl = 1, gh = 1, rt = 1; int B = 2, Bg = 1, Ts = 5, Hs = 100, Ws = 150, Tg = 7, t0 = 1,
            Td = 5, Hd = 64, Wd = 96, Ky = 4, Kx = 5; float eps = 1e-3f; int src_mis = 0, dst_mis = 0, tab_mis = 0; };
int fit(const Ft& p) {
    return drn_fit_frames(p.src ? (float*)A("src", (int64_t)p.B * p.Ts * p.Hs * p.Ws * 12, p.src_mis) : 0,
                          p.dst ? A("dst", (int64_t)p.B * 3 * p.Td * p.Hd * p.Wd * 2, p.dst_mis) : 0, p.B, p.Ts, p.Hs, p.Ws, p.Td, p.Hd, p.Wd,
                          p.tidx ? (int*)A("t_idx", p.Td * 4) : 0, p.ylo ? (int*)A("y_lo_n", p.Hd * 8) : 0,
                          p.yw ? (float*)A("y_w", (int64_t)p.Hd * p.Ky * 4, p.tab_mis) : 0, p.Ky, p.xlo ? (int*)A("x_lo_n", p.Wd * 8) : 0,
                          p.xw ? (float*)A("x_w", (int64_t)p.Wd * p.Kx * 4) : 0, p.Kx, STREAM);
}
int fit8(const Ft& p) {
    return drn_fit_frames_u8(p.src ? (uint8_t*)A("src", (int64_t)p.B * p.Ts * p.Hs * p.Ws * 3, p.src_mis) : 0,
                             p.dst ? A("dst", (int64_t)p.B * 3 * p.Td * p.Hd * p.Wd * 2, p.dst_mis) : 0, p.B, p.Ts, p.Hs, p.Ws, p.Td, p.Hd, p.Wd,
                             p.tidx ? (int*)A("t_idx", p.Td * 4) : 0, p.ylo ? (int*)A("y_lo_n", p.Hd * 8) : 0,
                             p.yw ? (float*)A("y_w", (int64_t)p.Hd * p.Ky * 4, p.tab_mis) : 0, p.Ky, p.xlo ? (int*)A("x_lo_n", p.Wd * 8) : 0,
                             p.xw ? (float*)A("x_w", (int64_t)p.Wd * p.Kx * 4) : 0, p.Kx, STREAM);
}
int rst(const Ft& p) {
    return drn_restore_frames_u8(p.src ? (uint8_t*)A("src", (int64_t)p.B * p.Ts * p.Hs * p.Ws * 3, p.src_mis) : 0,
                                 p.dst ? (uint8_t*)A("dst", (int64_t)p.B * p.Td * p.Hd * p.Wd * 3, p.dst_mis) : 0, p.B, p.Ts, p.Hs, p.Ws, p.Td, p.Hd,
                                 p.Wd, p.ylo ? (int*)A("y_lo_n", p.Hd * 8) : 0, p.yw ? (float*)A("y_w", (int64_t)p.Hd * p.Ky * 4, p.tab_mis) : 0, p.Ky,
                                 p.xlo ? (int*)A("x_lo_n", p.Wd * 8) : 0, p.xw ? (float*)A("x_w", (int64_t)p.Wd * p.Kx * 4) : 0, p.Kx, STREAM);
}
int rsg(const Ft& p) {
    return drn_restore_guided_u8(p.src ? (uint8_t*)A("src", (int64_t)p.B * p.Ts * p.Hs * p.Ws * 3, p.src_mis) : 0,
                                 p.gl ? (uint8_t*)A("guide_lo", (int64_t)p.Bg * p.Tg * p.Hs * p.Ws * 3) : 0,
                                 p.gh ? (uint8_t*)A("guide_hi", (int64_t)p.Bg * p.Tg * p.Hd * p.Wd * 3) : 0,
                                 p.dst ? (uint8_t*)A("dst", (int64_t)p.B * p.Td * p.Hd * p.Wd * 3, p.dst_mis) : 0, p.B, p.Bg, p.Ts, p.Hs, p.Ws, p.Tg,
                                 p.t0, p.Td, p.Hd, p.Wd, p.ylo ? (int*)A("y_lo_n", p.Hd * 8) : 0,
                                 p.yw ? (float*)A("y_w", (int64_t)p.Hd * p.Ky * 4, p.tab_mis) : 0, p.Ky, p.xlo ? (int*)A("x_lo_n", p.Wd * 8) : 0,
                                 p.xw ? (float*)A("x_w", (int64_t)p.Wd * p.Kx * 4) : 0, p.Kx, p.rt ? (float*)A("range_tab", 1024) : 0, p.eps, STREAM);
}

// ---- spatial tiles on uint8, latent tiles on bf16
struct Tl { bool canvas = 1, tile = 1, wy = 1, wx = 1, unc = 1, cur = 1, same = 0; int64_t frames = 57; int H = 704, W = 1280, h = 512, w = 513, y_at = 192, x_at = 767,
            ry = 3, rx = 5, Oy = 64, Ox = 65; int copies = 2; float sigma = 2.f; int mis = 0, w_mis = 0; };
int tb(const Tl& p) {
    return drn_tile_blend_u8(p.canvas ? A("canvas", p.frames * p.H * p.W * 3, p.mis) : 0, p.tile ? A("tile", p.frames * p.h * p.w * 3) : 0,
                             p.wy ? A("wy", p.Oy * 4, p.w_mis) : 0, p.wx ? A("wx", p.Ox * 4) : 0, p.frames, p.H, p.W, p.h, p.w, p.y_at, p.x_at, p.ry,
                             p.rx, p.Oy, p.Ox, STREAM);
}
int lg(const Tl& p) {
    return drn_latent_tile_gather(p.canvas ? A("canvas", p.frames * p.H * p.W * 2, p.mis) : 0,
                                  p.tile ? A("out", (int64_t)(p.copies > 0 ? p.copies : 1) * p.frames * p.h * p.w * 2) : 0, p.frames, p.H, p.W, p.h,
                                  p.w, p.y_at, p.x_at, 0.5f, p.copies, STREAM);
}
int lj(const Tl& p) {
    void* cur = p.cur ? A("canvas_cur", p.frames * p.H * p.W * 2) : 0;
    void* next = p.same ? cur : (p.canvas ? A("canvas_next", p.frames * p.H * p.W * 2, p.mis) : 0);
    return drn_latent_tile_step_join(p.tile ? A("model_out", p.frames * p.h * p.w * 2) : 0, p.unc ? A("uncond", p.frames * p.h * p.w * 2) : 0, 3.f,
                                     cur, next, p.wy ? (float*)A("wy", p.Oy * 4, p.w_mis) : 0, p.wx ? (float*)A("wx", p.Ox * 4) : 0, p.frames, p.H,
                                     p.W, p.h, p.w, p.y_at, p.x_at, p.ry, p.rx, p.Oy, p.Ox, 0.1f, 0.9f, p.sigma, -0.3f, STREAM);
}

// ---- seed ensembles: `members` is a HOST table the library reads - a heap block of exactly N pointers, so ASan guards it
struct En { bool members = 1, dst = 1, spread = 1, aff = 1, stats = 1, ws = 1; int null_member = -1, member_is_dst = -1, member_is_spread = -1; bool spread_is_dst = 0;
            int N = 5, B = 2, mode = 0; int64_t bytes = 3 * 1000 * 1000; int64_t ws_short = 0; int mis = 0, aff_mis = 0, st_mis = 0, ws_mis = 0; };
struct Members {
    const void** tab = nullptr;
    Members(const En& p, int64_t each, void* dst, void* spread) {
        if (!p.members || p.N < 1) return;
        tab = new const void*[p.N];
        for (int k = 0; k < p.N; ++k) {
            tab[k] = A("member", each, p.mis);
            if (k == p.null_member) tab[k] = nullptr;
            if (k == p.member_is_dst) tab[k] = dst;
            if (k == p.member_is_spread) tab[k] = spread;
        }
    }
    ~Members() { delete[] tab; }
};
int er(const En& p) {
    void* dst = p.dst ? A("dst", p.bytes) : 0;
    void* spread = p.spread_is_dst ? dst : (p.spread ? A("spread", p.bytes) : 0);
    Members m(p, p.bytes, dst, spread);
    return drn_ensemble_reduce_u8(m.tab, p.N, dst, spread, p.bytes, p.mode, STREAM);
}
int era(const En& p) {
    const int64_t all = p.B > 0 ? p.B * p.bytes : 0;
    void* dst = p.dst ? A("dst", all) : 0;
    void* spread = p.spread_is_dst ? dst : (p.spread ? A("spread", all) : 0);
    Members m(p, all, dst, spread);
    return drn_ensemble_reduce_affine_u8(m.tab, p.N, p.aff ? A("affine", (int64_t)p.N * p.B * 8, p.aff_mis) : 0, p.B, p.bytes, dst, spread, p.mode,
                                         STREAM);
}
int ea(const En& p) {
    const int64_t all = p.B > 0 ? p.B * p.bytes : 0, need = drn_ensemble_align_workspace_bytes(p.N, p.B, p.bytes) - p.ws_short;
    Members m(p, all, nullptr, nullptr);
    return drn_ensemble_align_affine(m.tab, p.N, p.B, p.bytes, p.aff ? A("affine", (int64_t)p.N * p.B * 8, p.aff_mis) : 0,
                                     p.stats ? A("stats", (int64_t)p.B * (p.N + p.N * p.N) * 8, p.st_mis) : 0,
                                     p.ws ? A("workspace", need, p.ws_mis) : 0, need, STREAM);
}

}  // namespace

void family_pictures() {
    entry<Pp>("drn_postprocess_u8", pp,
              {CH(Pp, "null video", p.v = 0), CH(Pp, "null out_u8", p.o = 0), CH(Pp, "B == 0", p.B = 0), CH(Pp, "T == 0", p.T = 0),
               CH(Pp, "H == 0", p.H = 0), CH(Pp, "W < 0", p.W = -8)},
              {CH(Pp, "H W % 8 != 0", (p.H = 45, p.W = 37)), CH(Pp, "video off the 16-byte grid", p.v_mis = 2), CH(Pp, "57 frames of 704 x 1280", (p.B = 1, p.T = 57, p.H = 704, p.W = 1280))},
              // D: bytes out = B T H W 3 either side of 2^31 and 2^32; frames either side of 65535
              {CH(Pp, "out 2^31 - 24 bytes", (p.B = 1, p.T = 1, p.H = 2, p.W = (int)(G / 3 - 4))), CH(Pp, "out past 2^31 bytes", (p.B = 1, p.T = 2, p.H = 32768, p.W = 16384)),
               CH(Pp, "out past 2^32 bytes", (p.B = 1, p.T = 3, p.H = 32768, p.W = 16384)), CH(Pp, "65535 frames", (p.B = 5, p.T = 13107, p.H = 8, p.W = 8)),
               CH(Pp, "65536 frames", (p.B = 4, p.T = 16384, p.H = 8, p.W = 8)), CH(Pp, "2^31 frames", (p.B = 32768, p.T = 65536, p.H = 1, p.W = 8)),
               CH(Pp, "one frame of 2^31 pixels", (p.B = 1, p.T = 1, p.H = 65536, p.W = 32768)), CH(Pp, "80 GiB in, 40 GiB out", (p.B = 4, p.T = 100, p.H = 8192, p.W = 4096))});

    const std::vector<Change<Pw>> pw_ref = {
        CH(Pw, "null video", p.v = 0), CH(Pw, "null out_u8", p.o = 0), CH(Pw, "prev_tail without ramp_w", p.rw = 0), CH(Pw, "ramp_w without prev_tail", p.prev = 0),
        CH(Pw, "O < 0", p.O = -1), CH(Pw, "ramp_at < 0", p.ramp_at = -1), CH(Pw, "ramp_at + O > Tw", p.ramp_at = 7), CH(Pw, "write_lo < 0", p.lo = -1),
        CH(Pw, "write_lo == write_hi", p.lo = 9), CH(Pw, "write_hi > Tw", p.hi = 10), CH(Pw, "write_lo inside the ramp", p.lo = 1),
        CH(Pw, "B == 0", p.B = 0), CH(Pw, "Tw == 0", p.Tw = 0), CH(Pw, "H == 0", p.H = 0), CH(Pw, "W == 0", p.W = 0),
        CH(Pw, "video off 2 bytes", p.v_mis = 1), CH(Pw, "prev_tail off 2 bytes", p.prev_mis = 1), CH(Pw, "ramp_w off 4 bytes", p.rw_mis = 2)};
    const std::vector<Change<Pw>> pw_ok = {CH(Pw, "no carry", (p.prev = 0, p.rw = 0, p.O = 0)), CH(Pw, "write behind the ramp", (p.lo = 3, p.hi = 8)),
                                           CH(Pw, "one pixel per lane", (p.H = 45, p.W = 37)), CH(Pw, "ramp in the middle, all written", p.ramp_at = 4)};
    const std::vector<Change<Pw>> pw_big = {CH(Pw, "window of 2^31 values per pass", (p.B = 1, p.Tw = 9, p.H = 8192, p.W = 16384, p.O = 1)),
                                            CH(Pw, "out past 2^32 bytes", (p.B = 2, p.Tw = 9, p.H = 16384, p.W = 16384, p.O = 1)),
                                            CH(Pw, "65536 written frames", (p.B = 8192, p.Tw = 9, p.lo = 1, p.hi = 9, p.H = 8, p.W = 8, p.O = 1))};
    entry<Pw>("drn_postprocess_window_u8", pw, pw_ref, pw_ok, pw_big);
    {
        auto r = pw_ref;
        r.push_back(CH(Pw, "affine off 4 bytes", p.aff_mis = 2));
        r.push_back(CH(Pw, "carry_out off 2 bytes", p.carry_mis = 1));
        r.push_back(CH(Pw, "carry_out with O == 0", (p.prev = 0, p.rw = 0, p.O = 0)));
        r.push_back(CH(Pw, "carry_out == prev_tail", p.carry_is = 1));
        r.push_back(CH(Pw, "carry_out == video", p.carry_is = 2));
        auto ok = pw_ok;
        ok[0] = CH(Pw, "no carry in or out", (p.prev = 0, p.rw = 0, p.O = 0, p.carry = 0));
        ok.push_back(CH(Pw, "no affine", p.aff = 0));
        ok.push_back(CH(Pw, "no carry_out", p.carry = 0));
        ok.push_back(CH(Pw, "first window: carry out, none in", (p.prev = 0, p.rw = 0)));
        entry<Pw>("drn_postprocess_window_align_u8", pwa, r, ok, pw_big);
    }

    entry<Wa>("drn_window_align_affine", wa,
              {CH(Wa, "null video", p.v = 0), CH(Wa, "null prev_tail", p.prev = 0), CH(Wa, "null affine", p.aff = 0), CH(Wa, "null workspace", p.ws = 0),
               CH(Wa, "O < 1", p.O = 0), CH(Wa, "ramp_at < 0", p.ramp_at = -1), CH(Wa, "ramp_at + O > Tw", p.ramp_at = 7),
               CH(Wa, "workspace one byte short", p.ws_short = 1), CH(Wa, "video off 2 bytes", p.v_mis = 1), CH(Wa, "prev_tail off 2 bytes", off("prev_tail", 1)), CH(Wa, "affine off 4 bytes", p.aff_mis = 2),
               CH(Wa, "moments off 8 bytes", p.mom_mis = 4), CH(Wa, "workspace off 8 bytes", p.ws_mis = 4), CH(Wa, "B == 0", p.B = 0), CH(Wa, "H == 0", p.H = 0),
               CH(Wa, "W == 0", p.W = 0), CH(Wa, "Tw == 0", p.Tw = 0), CH(Wa, "B > 65535", (p.B = 65536, p.H = 2, p.W = 2))},
              {CH(Wa, "no moments", p.mom = 0), CH(Wa, "one value per lane", (p.H = 45, p.W = 37)), CH(Wa, "B == 65535", (p.B = 65535, p.H = 2, p.W = 4))},
              {CH(Wa, "overlap of 2^31 values per channel", (p.B = 1, p.O = 8, p.Tw = 8, p.H = 16384, p.W = 16384)),
               CH(Wa, "overlap of 2^33 values per channel", (p.B = 1, p.O = 32, p.Tw = 32, p.H = 16384, p.W = 16384)),
               CH(Wa, "3 x 2^31 / 8192 chunks", (p.B = 1, p.O = 24, p.Tw = 24, p.H = 32768, p.W = 32768))});

    const std::vector<Change<Ev>> ev_ref = {CH(Ev, "null cube", p.cube = 0), CH(Ev, "null vec", p.vec = 0), CH(Ev, "null rot", p.rot = 0), CH(Ev, "null env_ldr", p.ldr = 0),
                                            CH(Ev, "null env_log", p.log = 0), CH(Ev, "R == 0", p.R = 0), CH(Ev, "T == 0", p.T = 0), CH(Ev, "H == 0", p.H = 0),
                                            CH(Ev, "W == 0", p.W = 0), CH(Ev, "cube off 4 bytes", p.mis = 2), CH(Ev, "vec off 4 bytes", off("vec", 2)), CH(Ev, "rot off 4 bytes", off("rot", 2)),
                                            CH(Ev, "env_ldr off 4 bytes", off("env_ldr", 2)), CH(Ev, "env_log off 4 bytes", off("env_log", 2))};
    {
        auto r = ev_ref;
        r.push_back(CH(Ev, "T H W == 2^31", (p.T = 8, p.H = 16384, p.W = 16384)));
        entry<Ev>("drn_env_project", ev, r, {CH(Ev, "T H W == 2^31 - 2^14", (p.T = 8, p.H = 16384, p.W = 16383)), CH(Ev, "one pixel", (p.T = 1, p.H = 1, p.W = 1))});
        r = ev_ref;
        r.push_back(CH(Ev, "null cube_of", p.cof = 0));
        r.push_back(CH(Ev, "n_cubes == 0", p.n_cubes = 0));
        r.push_back(CH(Ev, "t0 < 0", p.t0 = -1));
        r.push_back(CH(Ev, "t0 + T > T_all", p.t0 = 3));
        r.push_back(CH(Ev, "T_all H W == 2^31", (p.T_all = 8, p.H = 16384, p.W = 16384)));
        r.push_back(CH(Ev, "cube_of off 4 bytes", p.cof_mis = 2));
        entry<Ev>("drn_env_project_seq", evs, r, {CH(Ev, "the whole clip", (p.t0 = 0, p.T = 7)), CH(Ev, "T_all H W == 2^31 - 2^14", (p.T_all = 8, p.H = 16384, p.W = 16383))});
    }
    entry<Ec>("drn_env_cubes", ec,
              {CH(Ec, "null latlong", p.ll = 0), CH(Ec, "null grid", p.grid = 0), CH(Ec, "null cubes", p.cubes = 0), CH(Ec, "N == 0", p.N = 0),
               CH(Ec, "He == 0", p.He = 0), CH(Ec, "We == 0", p.We = 0), CH(Ec, "R == 0", p.R = 0), CH(Ec, "n0 < 0", p.n0 = -1), CH(Ec, "n == 0", p.n = 0),
               CH(Ec, "n0 + n > N", p.n0 = 3), CH(Ec, "roll < 0", p.roll = -1), CH(Ec, "roll == We", p.roll = 128), CH(Ec, "latlong off 4 bytes", p.mis = 2), CH(Ec, "grid off 4 bytes", off("grid", 2)), CH(Ec, "cubes off 4 bytes", off("cubes", 2)),
               CH(Ec, "N He We 3 == 2^31 + ...", (p.N = 4, p.n0 = 0, p.He = 8192, p.We = 32768)), CH(Ec, "n 6 R R 3 >= 2^31", (p.N = 32, p.n0 = 0, p.n = 32, p.R = 2048))},
              {CH(Ec, "roll == We - 1", p.roll = 127), CH(Ec, "2^31 - ... panorama values", (p.N = 2, p.n0 = 0, p.He = 8192, p.We = 32768)),
               CH(Ec, "n 6 R R 3 just below 2^31", (p.N = 28, p.n0 = 0, p.n = 28, p.R = 2048))});

    const std::vector<Change<Ft>> rs_ref = {CH(Ft, "null src", p.src = 0), CH(Ft, "null dst", p.dst = 0), CH(Ft, "null y_lo_n", p.ylo = 0), CH(Ft, "null y_w", p.yw = 0),
                                            CH(Ft, "null x_lo_n", p.xlo = 0), CH(Ft, "null x_w", p.xw = 0), CH(Ft, "B == 0", p.B = 0), CH(Ft, "Ts == 0", p.Ts = 0),
                                            CH(Ft, "Hs == 0", p.Hs = 0), CH(Ft, "Ws == 0", p.Ws = 0), CH(Ft, "Td == 0", p.Td = 0), CH(Ft, "Hd == 0", p.Hd = 0),
                                            CH(Ft, "Wd == 0", p.Wd = 0), CH(Ft, "Ky == 0", p.Ky = 0), CH(Ft, "Kx == 0", p.Kx = 0), CH(Ft, "a table off 4 bytes", p.tab_mis = 2), CH(Ft, "y_lo_n off 4 bytes", off("y_lo_n", 2)), CH(Ft, "x_lo_n off 4 bytes", off("x_lo_n", 2)), CH(Ft, "x_w off 4 bytes", off("x_w", 2))};
    {
        auto r = rs_ref;
        r.push_back(CH(Ft, "null t_idx", p.tidx = 0));
        r.push_back(CH(Ft, "t_idx off 4 bytes", off("t_idx", 2)));
        r.push_back(CH(Ft, "Ky == 33", p.Ky = 33));
        r.push_back(CH(Ft, "Kx == 33", p.Kx = 33));
        r.push_back(CH(Ft, "Hd % 16", p.Hd = 72));
        r.push_back(CH(Ft, "Wd % 16", p.Wd = 100));
        r.push_back(CH(Ft, "dst off 16 bytes", p.dst_mis = 8));
        r.push_back(CH(Ft, "dst past 2^31 elements", (p.B = 1, p.Td = 8, p.Hd = 8192, p.Wd = 10928)));
        r.push_back(CH(Ft, "src == 2^31 values", (p.B = 2, p.Ts = 8, p.Hs = 8192, p.Ws = 5462)));
        auto r32 = r, r8 = r;
        r32.push_back(CH(Ft, "src off 4 bytes", p.src_mis = 2));
        const std::vector<Change<Ft>> ok = {CH(Ft, "Ky == Kx == 32", (p.Ky = 32, p.Kx = 32)), CH(Ft, "Ky == Kx == 1", (p.Ky = 1, p.Kx = 1)),
                                            CH(Ft, "src just below 2^31 values", (p.B = 2, p.Ts = 8, p.Hs = 8192, p.Ws = 5461)),
                                            CH(Ft, "time padding: Td > Ts", p.Td = 9), CH(Ft, "dst just below 2^31 elements", (p.B = 1, p.Td = 8, p.Hd = 8192, p.Wd = 10912)), CH(Ft, "57 frames to 704 x 1280", (p.B = 1, p.Ts = 57, p.Td = 57, p.Hs = 1080, p.Ws = 1920, p.Hd = 704, p.Wd = 1280))};
        entry<Ft>("drn_fit_frames", fit, r32, ok);
        auto ok8 = ok;
        ok8.push_back(CH(Ft, "src at an odd byte", p.src_mis = 3));
        entry<Ft>("drn_fit_frames_u8", fit8, r8, ok8);

        r = rs_ref;
        r.push_back(CH(Ft, "Td > Ts", p.Td = 6));
        r.push_back(CH(Ft, "Ky == 33", p.Ky = 33));
        r.push_back(CH(Ft, "Kx == 33", p.Kx = 33));
        r.push_back(CH(Ft, "dst == 2^31 bytes", (p.B = 2, p.Ts = 8, p.Td = 8, p.Hd = 8192, p.Wd = 5462)));
        r.push_back(CH(Ft, "src == 2^31 bytes", (p.B = 2, p.Ts = 8, p.Hs = 8192, p.Ws = 5462, p.Td = 1)));
        entry<Ft>("drn_restore_frames_u8", rst, r,
                  {CH(Ft, "odd sizes and bases", (p.Hd = 101, p.Wd = 157, p.src_mis = 1, p.dst_mis = 3)), CH(Ft, "one output pixel", (p.Hd = 1, p.Wd = 1)),
                   CH(Ft, "dst just below 2^31 bytes", (p.B = 2, p.Ts = 8, p.Td = 8, p.Hd = 8192, p.Wd = 5461)),
                   CH(Ft, "src just below 2^31 bytes", (p.B = 2, p.Ts = 8, p.Hs = 8192, p.Ws = 5461, p.Td = 1))});
        r = rs_ref;
        r.push_back(CH(Ft, "null guide_lo", p.gl = 0));
        r.push_back(CH(Ft, "null guide_hi", p.gh = 0));
        r.push_back(CH(Ft, "null range_tab", p.rt = 0));
        r.push_back(CH(Ft, "range_tab off 4 bytes", off("range_tab", 2)));
        r.push_back(CH(Ft, "Bg == 0", p.Bg = 0));
        r.push_back(CH(Ft, "Bg neither 1 nor B", (p.B = 3, p.Bg = 2)));
        r.push_back(CH(Ft, "Tg == 0", p.Tg = 0));
        r.push_back(CH(Ft, "Td > Ts", (p.Td = 6, p.t0 = 0)));
        r.push_back(CH(Ft, "t0 < 0", p.t0 = -1));
        r.push_back(CH(Ft, "t0 + Td > Tg", p.t0 = 3));
        r.push_back(CH(Ft, "Ky == 9", p.Ky = 9));
        r.push_back(CH(Ft, "Kx == 9", p.Kx = 9));
        r.push_back(CH(Ft, "eps == 0", p.eps = 0.f));
        r.push_back(CH(Ft, "eps < 0", p.eps = -1.f));
        r.push_back(CH(Ft, "src == 2^31 bytes", (p.B = 2, p.Ts = 8, p.Tg = 8, p.t0 = 0, p.Td = 1, p.Hs = 8192, p.Ws = 5462, p.Hd = 4, p.Wd = 4)));
        r.push_back(CH(Ft, "guide_lo == 2^31 bytes", (p.B = 1, p.Ts = 1, p.Tg = 16, p.t0 = 0, p.Td = 1, p.Hs = 8192, p.Ws = 5462, p.Hd = 4, p.Wd = 4)));
        r.push_back(CH(Ft, "guide_hi == 2^31 bytes", (p.B = 1, p.Ts = 1, p.Tg = 16, p.t0 = 0, p.Td = 1, p.Hd = 8192, p.Wd = 5462, p.Hs = 4, p.Ws = 4)));
        r.push_back(CH(Ft, "dst == 2^31 bytes", (p.B = 2, p.Bg = 2, p.Ts = 8, p.Tg = 8, p.t0 = 0, p.Td = 8, p.Hd = 8192, p.Wd = 5462, p.Hs = 4, p.Ws = 4)));
        entry<Ft>("drn_restore_guided_u8", rsg, r,
                  {CH(Ft, "a guide per clip", p.Bg = 2), CH(Ft, "Ky == Kx == 8", (p.Ky = 8, p.Kx = 8)), CH(Ft, "odd sizes and bases", (p.Hd = 101, p.Wd = 157, p.src_mis = 1, p.dst_mis = 3)),
                   CH(Ft, "dst just below 2^31 bytes", (p.B = 2, p.Bg = 2, p.Ts = 8, p.Tg = 8, p.t0 = 0, p.Td = 8, p.Hd = 8192, p.Wd = 5461, p.Hs = 4, p.Ws = 4))});
    }

    const std::vector<Change<Tl>> tl_ref = {CH(Tl, "frames == 0", p.frames = 0), CH(Tl, "H == 0", p.H = 0), CH(Tl, "W == 0", p.W = 0), CH(Tl, "h == 0", p.h = 0),
                                            CH(Tl, "w == 0", p.w = 0), CH(Tl, "y_at < 0", p.y_at = -1), CH(Tl, "x_at < 0", p.x_at = -1), CH(Tl, "y_at + h > H", p.y_at = 193),
                                            CH(Tl, "x_at + w > W", p.x_at = 768)};
    const std::vector<Change<Tl>> bl_ref = {CH(Tl, "ry < 0", p.ry = -1), CH(Tl, "ry == h", (p.ry = 512, p.Oy = 0, p.wy = 0)), CH(Tl, "rx < 0", p.rx = -1),
                                            CH(Tl, "rx == w", (p.rx = 513, p.Ox = 0, p.wx = 0)), CH(Tl, "Oy < 0", p.Oy = -1), CH(Tl, "Ox < 0", p.Ox = -1),
                                            CH(Tl, "ry + Oy > h", p.Oy = 510), CH(Tl, "rx + Ox > w", p.Ox = 509), CH(Tl, "wy with Oy == 0", p.Oy = 0),
                                            CH(Tl, "Oy without wy", p.wy = 0), CH(Tl, "wx with Ox == 0", p.Ox = 0), CH(Tl, "Ox without wx", p.wx = 0),
                                            CH(Tl, "a weight table off 4 bytes", p.w_mis = 2), CH(Tl, "wx off 4 bytes", off("wx", 2))};
    {
        auto r = tl_ref;
        r.insert(r.end(), bl_ref.begin(), bl_ref.end());
        r.push_back(CH(Tl, "null canvas", p.canvas = 0));
        r.push_back(CH(Tl, "null tile", p.tile = 0));
        r.push_back(CH(Tl, "a canvas frame of 2^31 bytes", (p.frames = 1, p.H = 32768, p.W = 21846)));
        r.push_back(CH(Tl, "a tile frame of 2^31 bytes", (p.frames = 1, p.H = 32768, p.W = 32768, p.h = 32768, p.w = 21846, p.y_at = 0, p.x_at = 0)));
        r.push_back(CH(Tl, "2^31 workgroups", (p.frames = 2 * G, p.H = 16, p.W = 128, p.h = 16, p.w = 128, p.y_at = 0, p.x_at = 0, p.ry = 0, p.rx = 0, p.Oy = 4, p.Ox = 4)));
        entry<Tl>("drn_tile_blend_u8", tb, r,
                  {CH(Tl, "no ramps", (p.Oy = 0, p.Ox = 0, p.wy = 0, p.wx = 0)), CH(Tl, "canvas at an odd byte", p.mis = 1), CH(Tl, "the whole canvas", (p.h = 704, p.w = 1280, p.y_at = 0, p.x_at = 0)),
                   CH(Tl, "one written pixel", (p.ry = 511, p.rx = 512, p.Oy = 1, p.Ox = 1)),
                   // D: frame bases beyond 32 bits
                   CH(Tl, "canvas past 2^31 bytes", (p.frames = 800)), CH(Tl, "canvas past 2^32 bytes", (p.frames = 1600)),
                   CH(Tl, "canvas of 240 GB", (p.frames = 88000)), CH(Tl, "a canvas frame just below 2^31 bytes", (p.frames = 3, p.H = 32768, p.W = 21845)),
                   CH(Tl, "2^31 - 1 workgroups", (p.frames = 2 * G - 1, p.H = 16, p.W = 128, p.h = 16, p.w = 128, p.y_at = 0, p.x_at = 0, p.ry = 0, p.rx = 0, p.Oy = 4, p.Ox = 4))});

        r = tl_ref;
        r.push_back(CH(Tl, "null canvas", p.canvas = 0));
        r.push_back(CH(Tl, "null out", p.tile = 0));
        r.push_back(CH(Tl, "canvas at an odd byte", p.mis = 1));
        r.push_back(CH(Tl, "out at an odd byte", off("out", 1)));
        r.push_back(CH(Tl, "copies == 0", p.copies = 0));
        r.push_back(CH(Tl, "copies == 3", p.copies = 3));
        r.push_back(CH(Tl, "a canvas plane of 2^31 elements", (p.frames = 1, p.H = 32768, p.W = 65536)));
        r.push_back(CH(Tl, "2^30 workgroups per copy", (p.frames = G, p.H = 16, p.W = 128, p.h = 16, p.w = 128, p.y_at = 0, p.x_at = 0)));
        entry<Tl>("drn_latent_tile_gather", lg, r,
                  {CH(Tl, "one copy", p.copies = 1), CH(Tl, "canvas off the 16-byte grid", p.mis = 2), CH(Tl, "the whole canvas", (p.h = 704, p.w = 1280, p.y_at = 0, p.x_at = 0)),
                   CH(Tl, "canvas past 2^31 elements", p.frames = 2400), CH(Tl, "canvas past 2^32 elements", p.frames = 4800), CH(Tl, "canvas of 240 GB", p.frames = 133000),
                   CH(Tl, "a canvas plane just below 2^31 elements", (p.frames = 2, p.H = 32768, p.W = 65535)),
                   CH(Tl, "2^30 - 1 workgroups per copy", (p.frames = G - 1, p.H = 16, p.W = 128, p.h = 16, p.w = 128, p.y_at = 0, p.x_at = 0))});

        r = tl_ref;
        r.insert(r.end(), bl_ref.begin(), bl_ref.end());
        r.push_back(CH(Tl, "null model_out", p.tile = 0));
        r.push_back(CH(Tl, "null canvas_cur", p.cur = 0));
        r.push_back(CH(Tl, "null canvas_next", p.canvas = 0));
        r.push_back(CH(Tl, "canvas_cur == canvas_next", p.same = 1));
        r.push_back(CH(Tl, "canvas_next at an odd byte", p.mis = 1));
        r.push_back(CH(Tl, "canvas_cur at an odd byte", off("canvas_cur", 1)));
        r.push_back(CH(Tl, "model_out at an odd byte", off("model_out", 1)));
        r.push_back(CH(Tl, "uncond at an odd byte", off("uncond", 1)));
        r.push_back(CH(Tl, "sigma == 0", p.sigma = 0.f));
        r.push_back(CH(Tl, "a canvas plane of 2^31 elements", (p.frames = 1, p.H = 32768, p.W = 65536)));
        r.push_back(CH(Tl, "2^31 workgroups", (p.frames = 2 * G, p.H = 16, p.W = 128, p.h = 16, p.w = 128, p.y_at = 0, p.x_at = 0, p.ry = 0, p.rx = 0, p.Oy = 4, p.Ox = 4)));
        entry<Tl>("drn_latent_tile_step_join", lj, r,
                  {CH(Tl, "no CFG", p.unc = 0), CH(Tl, "no ramps", (p.Oy = 0, p.Ox = 0, p.wy = 0, p.wx = 0)), CH(Tl, "canvas past 2^31 elements", p.frames = 2400),
                   CH(Tl, "canvas past 2^32 elements", p.frames = 4800), CH(Tl, "canvases of 240 GB together", p.frames = 66000),
                   CH(Tl, "2^31 - 1 workgroups", (p.frames = 2 * G - 1, p.H = 16, p.W = 128, p.h = 16, p.w = 128, p.y_at = 0, p.x_at = 0, p.ry = 0, p.rx = 0, p.Oy = 4, p.Ox = 4))});
    }

    const std::vector<Change<En>> en_ref = {CH(En, "null members", p.members = 0), CH(En, "null member", p.null_member = 4), CH(En, "null dst", p.dst = 0),
                                            CH(En, "N == 0", p.N = 0), CH(En, "N == 17", p.N = 17), CH(En, "mode < 0", p.mode = -1), CH(En, "n_bytes < 0", p.bytes = -1),
                                            CH(En, "dst == spread", p.spread_is_dst = 1), CH(En, "dst is a member", p.member_is_dst = 2),
                                            CH(En, "spread is a member", p.member_is_spread = 0)};
    {
        auto r = en_ref;
        r.push_back(CH(En, "mode == 3", p.mode = 3));
        r.push_back(CH(En, "n_bytes % 3 in mode 2", (p.mode = 2, p.bytes = 1000)));
        entry<En>("drn_ensemble_reduce_u8", er, r,
                  {CH(En, "n_bytes == 0", p.bytes = 0), CH(En, "mean", p.mode = 1), CH(En, "normal", p.mode = 2), CH(En, "N == 1", p.N = 1), CH(En, "N == 16, normal", (p.N = 16, p.mode = 2)),
                   CH(En, "no spread", p.spread = 0), CH(En, "members off the 16-byte grid", p.mis = 5), CH(En, "one byte", p.bytes = 1),
                   CH(En, "n_bytes 2^31 - 1", p.bytes = 2 * G - 1), CH(En, "n_bytes 2^31", p.bytes = 2 * G), CH(En, "n_bytes 2^32 + 3, normal", (p.bytes = 4 * G + 3 - 1, p.mode = 2)),
                   CH(En, "16 members of 14 GiB (~250 GB)", (p.N = 16, p.bytes = 14 * G))});
        r = en_ref;
        r.push_back(CH(En, "mode == 2", (p.mode = 2)));
        r.push_back(CH(En, "B == 0", p.B = 0));
        r.push_back(CH(En, "affine off 4 bytes", p.aff_mis = 2));
        entry<En>("drn_ensemble_reduce_affine_u8", era, r,
                  {CH(En, "clip_bytes == 0", p.bytes = 0), CH(En, "mean", p.mode = 1), CH(En, "no affine", p.aff = 0), CH(En, "clip_bytes % 16 != 0", p.bytes = 1000003),
                   CH(En, "B == 1", p.B = 1), CH(En, "no spread", p.spread = 0), CH(En, "B 65536", (p.B = 65536, p.bytes = 48)),
                   CH(En, "clip_bytes 2^31", p.bytes = 2 * G), CH(En, "clip_bytes 2^32 + 16", p.bytes = 4 * G + 16), CH(En, "clip_bytes 2^36, N 2, B 1", (p.bytes = 64 * G, p.N = 2, p.B = 1, p.spread = 0))});
        entry<En>("drn_ensemble_align_affine", ea,
                  {CH(En, "null members", p.members = 0), CH(En, "null member", p.null_member = 4), CH(En, "null affine", p.aff = 0), CH(En, "null workspace", p.ws = 0),
                   CH(En, "N == 0", p.N = 0), CH(En, "N == 17", p.N = 17), CH(En, "B == 0", p.B = 0), CH(En, "B == 65536", (p.B = 65536, p.bytes = 48)),
                   CH(En, "clip_bytes == 0", p.bytes = 0), CH(En, "clip_bytes == 2^36 + 1", (p.bytes = 64 * G + 1, p.B = 1, p.N = 2)),
                   CH(En, "workspace one byte short", p.ws_short = 1), CH(En, "affine off 4 bytes", p.aff_mis = 2), CH(En, "stats off 8 bytes", p.st_mis = 4),
                   CH(En, "workspace off 8 bytes", p.ws_mis = 4)},
                  {CH(En, "N == 1", p.N = 1), CH(En, "N == 16", p.N = 16), CH(En, "no stats", p.stats = 0), CH(En, "members off the 16-byte grid", p.mis = 3),
                   CH(En, "B == 65535", (p.B = 65535, p.bytes = 48)), CH(En, "one byte", p.bytes = 1), CH(En, "clip_bytes 2^31 - 1", (p.bytes = 2 * G - 1, p.B = 1)),
                   CH(En, "clip_bytes 2^32 + 16", (p.bytes = 4 * G + 16, p.B = 1)), CH(En, "clip_bytes 2^36, N 3 (192 GiB)", (p.bytes = 64 * G, p.B = 1, p.N = 3))});
    }
}

}  // namespace hw
