// host walk, the tokenizer family: implicit-GEMM convolution, group norm, Haar patching, resampling, the mid-block attention pieces,
// layout moves.  Sections A and D of the walk for these entries.
#include "host_walk.h"

namespace hw {
namespace {

// ---- drn_conv3d_igemm
struct Cv {
    bool x = 1, w = 1, bias = 1, y = 1, res = 1;
    int T = 3, H = 32, W = 32, C = 128, ih = 1, N = 128, kT = 3, kH = 3, kW = 3, sT = 1, sH = 1, sW = 1, pad = 1, t_off = 2, To = 3, Ho = 32, Wo = 32, oh = 1;
    int64_t ldc = 128, ldr = 128;
    int f32 = 0, x_mis = 0, w_mis = 0, y_mis = 0;
};
int cv(const Cv& p) {
    const int64_t ypix = (int64_t)p.To * (p.Ho + 2 * p.oh) * (p.Wo + 2 * p.oh);
    return drn_conv3d_igemm(p.x ? A("x", (int64_t)p.T * (p.H + 2 * p.ih) * (p.W + 2 * p.ih) * p.C * 2, p.x_mis) : 0,
                            p.w ? A("w", (int64_t)p.N * p.kT * p.kH * p.kW * p.C * 2, p.w_mis) : 0, p.bias ? A("bias", p.N * 2) : 0,
                            p.y ? A("y", ypix * p.ldc * (p.f32 ? 4 : 2), p.y_mis) : 0, p.res ? A("residual", ypix * p.ldr * 2) : 0, p.T, p.H, p.W, p.C, p.ih, p.N,
                            p.kT, p.kH, p.kW, p.sT, p.sH, p.sW, p.pad, p.t_off, p.To, p.Ho, p.Wo, p.oh, p.ldc, p.ldr, p.f32, 1.f, STREAM);
}

// ---- group norm
struct Gn { bool x = 1, g = 1, b = 1, y = 1, ws = 1; int frames = 3, H = 32, W = 32, C = 128, halo = 1, nparts = 8; float count = 32.f * 32 * 128 * 8; };
int64_t cl_bytes(int T, int H, int W, int C, int halo) { return (int64_t)T * (H + 2 * halo) * (W + 2 * halo) * C * 2; }
int gn(const Gn& p) {
    return drn_groupnorm_silu(p.x ? A("x", cl_bytes(p.frames, p.H, p.W, p.C, p.halo)) : 0, p.g ? A("gamma", p.C * 2) : 0, p.b ? A("beta", p.C * 2) : 0,
                              p.y ? A("y", cl_bytes(p.frames, p.H, p.W, p.C, p.halo)) : 0, p.ws ? A("workspace", drn_groupnorm_workspace_bytes(p.frames)) : 0,
                              p.frames, p.H, p.W, p.C, p.halo, 1e-6f, 1, STREAM);
}
int gns(const Gn& p) {
    return drn_groupnorm_stats(p.x ? A("x", cl_bytes(p.frames, p.H, p.W, p.C, p.halo)) : 0, p.ws ? A("part", (int64_t)p.frames * 64 * 16) : 0, p.frames, p.H, p.W,
                               p.C, p.halo, STREAM);
}
int gna(const Gn& p) {
    return drn_groupnorm_apply(p.x ? A("x", cl_bytes(p.frames, p.H, p.W, p.C, p.halo)) : 0, p.ws ? A("part", (int64_t)p.frames * p.nparts * 16) : 0, p.nparts,
                               p.count, p.g ? A("gamma", p.C * 2) : 0, p.b ? A("beta", p.C * 2) : 0, p.y ? A("y", cl_bytes(p.frames, p.H, p.W, p.C, p.halo)) : 0,
                               p.frames, p.H, p.W, p.C, p.halo, 1e-6f, 1, STREAM);
}

// ---- Haar patching
struct Hp { bool a = 1, b = 1; int Cin = 3, T = 9, H = 64, W = 96, halo = 1; };
int hp(const Hp& p) {
    return drn_haar_patch(p.a ? A("video", (int64_t)p.Cin * p.T * p.H * p.W * 2) : 0, p.b ? A("out", cl_bytes((p.T + 3) / 4, p.H / 4, p.W / 4, 64 * p.Cin, p.halo)) : 0,
                          p.Cin, p.T, p.H, p.W, p.halo, STREAM);
}
struct Hu { bool a = 1, b = 1; int C = 3, Tp = 3, Hq = 16, Wq = 24, halo = 1; };
int hu(const Hu& p) {
    return drn_haar_unpatch(p.a ? A("patches", cl_bytes(p.Tp, p.Hq, p.Wq, 64 * p.C, p.halo)) : 0,
                            p.b ? A("video", (int64_t)p.C * (4 * p.Tp - 3) * 4 * p.Hq * 4 * p.Wq * 2) : 0, p.C, p.Tp, p.Hq, p.Wq, p.halo, STREAM);
}

// ---- resample
struct Rs { bool x = 1, y = 1; int mode = 0, T = 5, H = 32, W = 48, C = 128, To = 5, Ho = 16, Wo = 24, halo = 1; };
int rs(const Rs& p) {
    return drn_resample(p.x ? A("x", cl_bytes(p.T, p.H, p.W, p.C, p.halo)) : 0, p.y ? A("y", cl_bytes(p.To, p.Ho, p.Wo, p.C, p.halo)) : 0, p.mode, p.T, p.H, p.W,
                        p.C, p.To, p.Ho, p.Wo, p.halo, STREAM);
}

// ---- mid-block attention pieces
struct Sx { bool s = 1, pr = 1; int64_t rows = 9216; int n = 9216; int64_t ld = 9216, ldp = 9216; };
int sx(const Sx& p) { return drn_softmax_rows(p.s ? A("scores", p.rows * p.ld * 4) : 0, p.pr ? A("probs", p.rows * p.ldp * 2) : 0, p.rows, p.n, p.ld, p.ldp, STREAM); }
int sxs(const Sx& p) {
    return drn_softmax_rows_scaled(p.s ? A("scores", p.rows * p.ld * 4) : 0, p.pr ? A("probs", p.rows * p.ldp * 2) : 0, p.rows, p.n, p.ld, p.ldp, 0.044f, STREAM);
}
struct Tr { bool x = 1, y = 1; int rows = 9216, cols = 512; int64_t ldx = 1536, ldo = 9216; };
int tr(const Tr& p) {
    return drn_transpose_bf16(p.x ? A("x", ((p.rows - 1) * p.ldx + p.cols) * 2) : 0, p.y ? A("y", ((p.cols - 1) * p.ldo + p.rows) * 2) : 0, p.rows, p.cols, p.ldx,
                              p.ldo, STREAM);
}
struct Ta { bool q = 1, k = 1, v = 1, o = 1; int T = 5; int64_t P = 9216; int C = 512; };
int ta(const Ta& p) {
    const int64_t n = (int64_t)p.T * p.P * p.C * 2;
    return drn_temporal_attention(p.q ? A("q", n) : 0, p.k ? A("k", n) : 0, p.v ? A("v", n) : 0, p.o ? A("o", n) : 0, p.T, p.P, p.C, 0.044f, STREAM);
}

// ---- layout moves
struct Lm { bool x = 1, y = 1; int C = 16, T = 5, H = 88, W = 160, Cs = 64, halo = 1; };
int p2c(const Lm& p) {
    return drn_planar_to_cl(p.x ? A("x", (int64_t)p.C * p.T * p.H * p.W * 2) : 0, p.y ? A("y", cl_bytes(p.T, p.H, p.W, p.Cs, p.halo)) : 0, p.C, p.T, p.H, p.W, p.Cs,
                            p.halo, STREAM);
}
int c2p(const Lm& p) {
    return drn_cl_to_planar(p.x ? A("x", cl_bytes(p.T, p.H, p.W, p.Cs, p.halo)) : 0, p.y ? A("y", (int64_t)p.C * p.T * p.H * p.W * 2) : 0, p.C, p.T, p.H, p.W, p.Cs,
                            p.halo, STREAM);
}

}  // namespace

void family_vae() {
    entry<Cv>("drn_conv3d_igemm", cv,
              {CH(Cv, "null x", p.x = 0), CH(Cv, "null w", p.w = 0), CH(Cv, "null y", p.y = 0), CH(Cv, "T == 0", p.T = 0), CH(Cv, "H == 0", p.H = 0), CH(Cv, "W == 0", p.W = 0),
               CH(Cv, "C % 64", p.C = 96), CH(Cv, "C == 0", p.C = 0), CH(Cv, "N % 4", p.N = 126), CH(Cv, "N == 0", p.N = 0), CH(Cv, "kT == 0", p.kT = 0), CH(Cv, "kH == 0", p.kH = 0),
               CH(Cv, "kW == 0", p.kW = 0), CH(Cv, "sT == 0", p.sT = 0), CH(Cv, "sH == 0", p.sH = 0), CH(Cv, "sW == 0", p.sW = 0), CH(Cv, "pad 2", p.pad = 2), CH(Cv, "To == 0", p.To = 0),
               CH(Cv, "Ho == 0", p.Ho = 0), CH(Cv, "Wo == 0", p.Wo = 0), CH(Cv, "ldc < N", p.ldc = 64), CH(Cv, "ldc % 4", p.ldc = 130), CH(Cv, "ldr < N", p.ldr = 64),
               CH(Cv, "ldr % 4", p.ldr = 130), CH(Cv, "out_f32 with a residual", p.f32 = 1), CH(Cv, "in_halo 2", p.ih = 2), CH(Cv, "pad without a halo", p.ih = 0),
               CH(Cv, "a tap below the image", p.Ho = 33), CH(Cv, "a tap right of the image", p.Wo = 33), CH(Cv, "a tap behind the last frame", p.To = 4),
               CH(Cv, "x off 16 bytes", p.x_mis = 8), CH(Cv, "w off 16 bytes", p.w_mis = 8), CH(Cv, "y off 8 bytes", p.y_mis = 4),
               CH(Cv, "strides whose tap row overflows an int", (p.Ho = 1 << 20, p.sH = 1 << 12))},
              {CH(Cv, "no bias, no residual", (p.bias = 0, p.res = 0)), CH(Cv, "fp32 output", (p.f32 = 1, p.res = 0)), CH(Cv, "1x1x1 as a dense GEMM", (p.kT = p.kH = p.kW = 1, p.pad = 0, p.t_off = 0, p.ih = 0, p.oh = 0)),
               CH(Cv, "stride 2", (p.sH = 2, p.sW = 2, p.Ho = 16, p.Wo = 16, p.pad = 0, p.kH = 2, p.kW = 2, p.ih = 0)),
               CH(Cv, "the big decoder conv: the 256 x 256 kernel", (p.T = 8, p.H = 176, p.W = 320, p.C = 256, p.N = 256, p.To = 8, p.Ho = 176, p.Wo = 320, p.ldc = 256, p.ldr = 256)),
               CH(Cv, "N 12: the last conv", (p.N = 12, p.ldc = 12, p.ldr = 12))},
              {CH(Cv, "input past 2^32 bytes", (p.T = 33, p.H = 704, p.W = 1280, p.C = 128, p.To = 33, p.Ho = 704, p.Wo = 1280, p.t_off = 2)),
               CH(Cv, "input past 2^32 bytes, 256 channels", (p.T = 17, p.H = 704, p.W = 1280, p.C = 256, p.N = 256, p.ldc = 256, p.ldr = 256, p.To = 17, p.Ho = 704, p.Wo = 1280)),
               CH(Cv, "2^31 output positions", (p.T = 2048, p.H = 1024, p.W = 1024, p.C = 64, p.N = 4, p.ldc = 4, p.ldr = 4, p.To = 2048, p.Ho = 1024, p.Wo = 1024, p.kT = 1, p.t_off = 0))});

    const std::vector<Change<Gn>> gn_ref = {CH(Gn, "null x", p.x = 0), CH(Gn, "frames == 0", p.frames = 0), CH(Gn, "frames > 65535", (p.frames = 65536, p.H = 2, p.W = 2, p.C = 8)),
                                            CH(Gn, "H == 0", p.H = 0), CH(Gn, "W == 0", p.W = 0), CH(Gn, "C == 0", p.C = 0), CH(Gn, "C % 8", p.C = 100), CH(Gn, "halo 2", p.halo = 2)};
    {
        auto r = gn_ref;
        r.push_back(CH(Gn, "null gamma", p.g = 0));
        r.push_back(CH(Gn, "null beta", p.b = 0));
        r.push_back(CH(Gn, "null y", p.y = 0));
        r.push_back(CH(Gn, "null workspace", p.ws = 0));
        const std::vector<Change<Gn>> ok = {CH(Gn, "compact", p.halo = 0), CH(Gn, "65535 frames", (p.frames = 65535, p.H = 2, p.W = 2, p.C = 8)),
                                            CH(Gn, "the decoder's last stage", (p.frames = 57, p.H = 704, p.W = 1280, p.C = 128))};
        const std::vector<Change<Gn>> big = {CH(Gn, "a frame of 2^31 elements", (p.frames = 2, p.H = 4096, p.W = 4096, p.C = 128)),
                                             CH(Gn, "a frame of 2^32 elements", (p.frames = 2, p.H = 8192, p.W = 4096, p.C = 128))};
        entry<Gn>("drn_groupnorm_silu", gn, r, ok, big);
        auto rs_ = gn_ref;
        rs_.push_back(CH(Gn, "null part", p.ws = 0));
        entry<Gn>("drn_groupnorm_stats", gns, rs_, ok, big);
        r.back() = CH(Gn, "null part", p.ws = 0);
        r.push_back(CH(Gn, "nparts == 0", p.nparts = 0));
        r.push_back(CH(Gn, "count == 0", p.count = 0.f));
        entry<Gn>("drn_groupnorm_apply", gna, r, ok, big);
    }
    entry<Hp>("drn_haar_patch", hp,
              {CH(Hp, "null video", p.a = 0), CH(Hp, "null out", p.b = 0), CH(Hp, "Cin == 0", p.Cin = 0), CH(Hp, "T == 0", p.T = 0), CH(Hp, "H == 0", p.H = 0), CH(Hp, "W == 0", p.W = 0),
               CH(Hp, "H % 4", p.H = 66), CH(Hp, "W % 4", p.W = 98), CH(Hp, "(T + 3) % 4", p.T = 8)},
              {CH(Hp, "one frame", p.T = 1), CH(Hp, "compact", p.halo = 0), CH(Hp, "57 frames of 704 x 1280", (p.T = 57, p.H = 704, p.W = 1280))},
              {CH(Hp, "a clip past 2^31 elements", (p.T = 257, p.H = 2048, p.W = 2048)), CH(Hp, "a clip past 2^32 elements", (p.T = 513, p.H = 2048, p.W = 2048))});
    entry<Hu>("drn_haar_unpatch", hu,
              {CH(Hu, "null patches", p.a = 0), CH(Hu, "null video", p.b = 0), CH(Hu, "Cimg == 0", p.C = 0), CH(Hu, "Tp == 0", p.Tp = 0), CH(Hu, "Hq == 0", p.Hq = 0), CH(Hu, "Wq == 0", p.Wq = 0)},
              {CH(Hu, "one frame", p.Tp = 1), CH(Hu, "15 x 176 x 320", (p.Tp = 15, p.Hq = 176, p.Wq = 320))},
              {CH(Hu, "a clip past 2^32 elements", (p.Tp = 129, p.Hq = 512, p.Wq = 512))});
    entry<Rs>("drn_resample", rs,
              {CH(Rs, "null x", p.x = 0), CH(Rs, "null y", p.y = 0), CH(Rs, "mode 4", p.mode = 4), CH(Rs, "mode -1", p.mode = -1), CH(Rs, "T == 0", p.T = 0), CH(Rs, "C % 8", p.C = 100),
               CH(Rs, "halo 2", p.halo = 2), CH(Rs, "mode 0 compact", p.halo = 0), CH(Rs, "mode 0 with odd H", (p.H = 33, p.Ho = 16)), CH(Rs, "mode 0 with the wrong Ho", p.Ho = 32),
               CH(Rs, "mode 1 with the wrong To", (p.mode = 1, p.To = 5, p.Ho = 32, p.Wo = 48)), CH(Rs, "mode 2 with the wrong To", (p.mode = 2, p.To = 10, p.Ho = 32, p.Wo = 48)),
               CH(Rs, "mode 3 with the wrong Wo", (p.mode = 3, p.To = 5, p.Ho = 64, p.Wo = 48))},
              {CH(Rs, "mode 1", (p.mode = 1, p.To = 3, p.Ho = 32, p.Wo = 48)), CH(Rs, "mode 2", (p.mode = 2, p.To = 9, p.Ho = 32, p.Wo = 48)),
               CH(Rs, "mode 2, one frame", (p.mode = 2, p.T = 1, p.To = 1, p.Ho = 32, p.Wo = 48)), CH(Rs, "mode 3", (p.mode = 3, p.To = 5, p.Ho = 64, p.Wo = 96))},
              {CH(Rs, "mode 3 to 2^32 elements", (p.mode = 3, p.T = 32, p.To = 32, p.H = 512, p.W = 1024, p.Ho = 1024, p.Wo = 2048, p.C = 64))});

    const std::vector<Change<Sx>> sx_ref = {CH(Sx, "null scores", p.s = 0), CH(Sx, "null probs", p.pr = 0), CH(Sx, "rows < 0", p.rows = -1), CH(Sx, "n == 0", p.n = 0),
                                            CH(Sx, "ld < n", p.ld = 9000), CH(Sx, "ldp < n", p.ldp = 9000), CH(Sx, "rows == 2^31", (p.rows = 1ll << 31, p.n = 8, p.ld = 8, p.ldp = 8))};
    const std::vector<Change<Sx>> sx_ok = {CH(Sx, "rows == 0", p.rows = 0), CH(Sx, "one column", (p.n = 1, p.ld = 1, p.ldp = 1)), CH(Sx, "rows == 2^31 - 1", (p.rows = (1ll << 31) - 1, p.n = 8, p.ld = 8, p.ldp = 8)),
                                           CH(Sx, "2^32 scores", (p.rows = 65536, p.n = 65536, p.ld = 65536, p.ldp = 65536))};
    entry<Sx>("drn_softmax_rows", sx, sx_ref, sx_ok);
    entry<Sx>("drn_softmax_rows_scaled", sxs, sx_ref, sx_ok);
    entry<Tr>("drn_transpose_bf16", tr,
              {CH(Tr, "null x", p.x = 0), CH(Tr, "null y", p.y = 0), CH(Tr, "rows == 0", p.rows = 0), CH(Tr, "cols == 0", p.cols = 0), CH(Tr, "ldx < cols", p.ldx = 500), CH(Tr, "ldo < rows", p.ldo = 9000),
               CH(Tr, "ldo == 65535 * 32 + 1: 65536 row tiles", (p.rows = 1, p.cols = 1, p.ldx = 1, p.ldo = 65535 * 32 + 1)),
               CH(Tr, "cols == 2^31 - 31", (p.rows = 1, p.cols = 0x7fffffff - 30, p.ldx = 0x7fffffff, p.ldo = 1))},
              {CH(Tr, "ldo == 65535 * 32: 65535 row tiles", (p.rows = 1, p.cols = 1, p.ldx = 1, p.ldo = 65535 * 32)),
               CH(Tr, "cols == 2^31 - 32", (p.rows = 1, p.cols = 0x7fffffff - 31, p.ldx = 0x7fffffff, p.ldo = 1)), CH(Tr, "one element", (p.rows = 1, p.cols = 1)), CH(Tr, "odd sizes", (p.rows = 333, p.cols = 77, p.ldx = 77, p.ldo = 333))},
              {CH(Tr, "2^32 elements", (p.rows = 65536, p.cols = 65536, p.ldx = 65536, p.ldo = 65536)), CH(Tr, "2^31 - 1 rows of one", (p.rows = 0x7fffffff, p.cols = 1, p.ldx = 1, p.ldo = 0x7fffffff)),
               CH(Tr, "one row of 2^31 - 1", (p.rows = 1, p.cols = 0x7fffffff, p.ldx = 0x7fffffff, p.ldo = 1))});
    entry<Ta>("drn_temporal_attention", ta,
              {CH(Ta, "null q", p.q = 0), CH(Ta, "null k", p.k = 0), CH(Ta, "null v", p.v = 0), CH(Ta, "null o", p.o = 0), CH(Ta, "T == 0", p.T = 0), CH(Ta, "T > 16", p.T = 17),
               CH(Ta, "P == 0", p.P = 0), CH(Ta, "C == 0", p.C = 0), CH(Ta, "C % 8", p.C = 500), CH(Ta, "P == 2^33 - 3: 2^31 workgroups", (p.T = 1, p.P = (1ll << 33) - 3, p.C = 8))},
              {CH(Ta, "P == 2^33 - 4: 2^31 - 1 workgroups", (p.T = 1, p.P = (1ll << 33) - 4, p.C = 8)), CH(Ta, "T 16", p.T = 16), CH(Ta, "one position", p.P = 1)},
              {CH(Ta, "2^31 elements", (p.T = 8, p.P = 1 << 19, p.C = 512)), CH(Ta, "2^33 positions", (p.T = 1, p.P = 1ll << 33, p.C = 8)), CH(Ta, "2^36 elements (128 GiB each)", (p.T = 16, p.P = 1ll << 23, p.C = 512))});
    const std::vector<Change<Lm>> lm_ref = {CH(Lm, "null x", p.x = 0), CH(Lm, "null y", p.y = 0), CH(Lm, "C == 0", p.C = 0), CH(Lm, "T == 0", p.T = 0), CH(Lm, "H == 0", p.H = 0), CH(Lm, "W == 0", p.W = 0),
                                            CH(Lm, "Cs < C", p.Cs = 8), CH(Lm, "halo 2", p.halo = 2)};
    const std::vector<Change<Lm>> lm_ok = {CH(Lm, "compact, Cs == C", (p.halo = 0, p.Cs = 16)), CH(Lm, "one element", (p.C = 1, p.T = 1, p.H = 1, p.W = 1, p.Cs = 1))};
    const std::vector<Change<Lm>> lm_big = {CH(Lm, "2^31 elements", (p.C = 64, p.T = 32, p.H = 1024, p.W = 1024, p.Cs = 64)), CH(Lm, "2^33 elements", (p.C = 128, p.T = 64, p.H = 1024, p.W = 1024, p.Cs = 128))};
    entry<Lm>("drn_planar_to_cl", p2c, lm_ref, lm_ok, lm_big);
    entry<Lm>("drn_cl_to_planar", c2p, lm_ref, lm_ok, lm_big);
}

}  // namespace hw
