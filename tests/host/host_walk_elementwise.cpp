// host walk, the elementwise family: norms, modulates, RoPE, patchify, sampler steps, step cache, GEMV, MX quantise.
// Sections A (refusals one at a time) and D (sizes we never run) of the walk for these entries.
#include "host_walk.h"

namespace hw {
namespace {

const int64_t G = 1ll << 30;

// ---- drn_rmsnorm
struct Rms { bool x = 1, w = 1, y = 1; int64_t rows = 300, D = 4096; };
int rms(const Rms& p) {
    return drn_rmsnorm(p.x ? A("x", p.rows * p.D * 2) : 0, p.w ? A("w", p.D * 2) : 0, p.y ? A("y", p.rows * p.D * 2) : 0, p.rows, p.D,
                       1e-6f, STREAM);
}

// ---- drn_ln_modulate / _mx
struct Ln { bool x = 1, add = 1, shift = 1, scale = 1, h = 1, hq = 1, hs = 1; int64_t rows = 512, D = 4096, rpb = 256; int hq_mis = 0; };
int ln(const Ln& p) {
    const int64_t nb = p.rpb > 0 ? (p.rows + p.rpb - 1) / p.rpb : 1;
    return drn_ln_modulate(p.x ? A("x", p.rows * p.D * 2) : 0, p.add ? A("add", nb * p.D * 2) : 0, p.shift ? A("shift", nb * p.D * 2) : 0,
                           p.scale ? A("scale", nb * p.D * 2) : 0, p.h ? A("h", p.rows * p.D * 2) : 0, p.rows, p.D, p.rpb, 1e-6f, STREAM);
}
int ln_mx(const Ln& p) {
    const int64_t nb = p.rpb > 0 ? (p.rows + p.rpb - 1) / p.rpb : 1;
    return drn_ln_modulate_mx(p.x ? A("x", p.rows * p.D * 2) : 0, p.add ? A("add", nb * p.D * 2) : 0, p.shift ? A("shift", nb * p.D * 2) : 0,
                              p.scale ? A("scale", nb * p.D * 2) : 0, p.h ? A("h", p.rows * p.D * 2) : 0,
                              p.hq ? A("hq", p.rows * p.D, p.hq_mis) : 0, p.hs ? A("hs", p.rows * p.D / 32) : 0, p.rows, p.D, p.rpb, 1e-6f,
                              STREAM);
}

// ---- drn_splitk_gate_res_ln_modulate / _mx
struct Sk { bool part = 1, x = 1, gate = 1, add = 1, shift = 1, scale = 1, h = 1, hq = 1, hs = 1; int splits = 4;
            int64_t rows = 256, D = 4096, rpb = 256; int part_mis = 0, hq_mis = 0; };
int sk(const Sk& p) {
    const int64_t nb = p.rpb > 0 ? (p.rows + p.rpb - 1) / p.rpb : 1, v = nb * p.D * 2;
    return drn_splitk_gate_res_ln_modulate(p.part ? A("partials", (int64_t)p.splits * p.rows * p.D * 4, p.part_mis) : 0, p.splits,
                                           p.x ? A("x", p.rows * p.D * 2) : 0, p.gate ? A("gate", v) : 0, p.add ? A("add", v) : 0,
                                           p.shift ? A("shift", v) : 0, p.scale ? A("scale", v) : 0, p.h ? A("h", p.rows * p.D * 2) : 0,
                                           p.rows, p.D, p.rpb, 1e-6f, STREAM);
}
int sk_mx(const Sk& p) {
    const int64_t nb = p.rpb > 0 ? (p.rows + p.rpb - 1) / p.rpb : 1, v = nb * p.D * 2;
    return drn_splitk_gate_res_ln_modulate_mx(p.part ? A("partials", (int64_t)p.splits * p.rows * p.D * 4, p.part_mis) : 0, p.splits,
                                              p.x ? A("x", p.rows * p.D * 2) : 0, p.gate ? A("gate", v) : 0, p.add ? A("add", v) : 0,
                                              p.shift ? A("shift", v) : 0, p.scale ? A("scale", v) : 0,
                                              p.h ? A("h", p.rows * p.D * 2) : 0, p.hq ? A("hq", p.rows * p.D, p.hq_mis) : 0,
                                              p.hs ? A("hs", p.rows * p.D / 32) : 0, p.rows, p.D, p.rpb, 1e-6f, STREAM);
}

// ---- drn_bcast_add
struct Bc { bool x = 1, v = 1; int64_t rows = 512, D = 4096, rpb = 256; };
int bc(const Bc& p) {
    const int64_t nb = p.rpb > 0 ? (p.rows + p.rpb - 1) / p.rpb : 1;
    return drn_bcast_add(p.x ? A("x", p.rows * p.D * 2) : 0, p.v ? A("vec", nb * p.D * 2) : 0, p.rows, p.D, p.rpb, STREAM);
}

// ---- drn_permute_021
struct Pm { bool x = 1, y = 1, same = 0; int64_t a = 2304, b = 8, c = 512; int mis = 0, y_mis = 0; };
int pm(const Pm& p) {
    void* x = p.x ? A("x", p.a * p.b * p.c * 2, p.mis) : 0;
    void* y = p.same ? x : (p.y ? A("y", p.a * p.b * p.c * 2, p.y_mis) : 0);
    return drn_permute_021(x, y, p.a, p.b, p.c, STREAM);
}

// ---- drn_qk_norm_rope / _mx
struct Qk { bool q = 1, k = 1, wq = 1, wk = 1, cos = 1, sin = 1, qq = 1, qs = 1, kq = 1, ks = 1; int64_t tokens = 512; int heads = 16;
            int64_t ldq = 3 * 2048, ldk = 3 * 2048, tpb = 256, pos = 0; int wb = 0, q_mis = 0, qq_mis = 0, k_mis = 0, kq_mis = 0; };   // q_mis moves the shared arena, k_mis k alone
int qk(const Qk& p) {
    // q and k are views into the fused QKV output: one arena, k at column D
    const int64_t D = (int64_t)p.heads * 128;
    char* qkv = (char*)A("qkv", p.tokens * p.ldq * 2, p.q_mis);
    return drn_qk_norm_rope(p.q ? qkv : 0, p.k ? qkv + D * 2 + p.k_mis : 0, p.wq ? A("wq", 256) : 0, p.wk ? A("wk", 256) : 0,
                            p.cos ? A("cos", (p.pos + p.tpb) * 256) : 0, p.sin ? A("sin", (p.pos + p.tpb) * 256) : 0, p.tokens, p.heads,
                            p.ldq, p.ldk, p.tpb, p.pos, 1e-6f, STREAM);
}
int qk_mx(const Qk& p) {
    const int64_t D = (int64_t)p.heads * 128;
    char* qkv = (char*)A("qkv", p.tokens * p.ldq * 2, p.q_mis);
    return drn_qk_norm_rope_mx(p.q ? qkv : 0, p.k ? qkv + D * 2 + p.k_mis : 0, p.wq ? A("wq", 256) : 0, p.wk ? A("wk", 256) : 0,
                               p.cos ? A("cos", (p.pos + p.tpb) * 256) : 0, p.sin ? A("sin", (p.pos + p.tpb) * 256) : 0,
                               p.qq ? A("qq", p.tokens * D, p.qq_mis) : 0, p.qs ? A("qs", p.tokens * D / 32) : 0,
                               p.kq ? A("kq", p.tokens * D, p.kq_mis) : 0, p.ks ? A("ks", p.tokens * D / 32) : 0, p.tokens, p.heads, p.ldq, p.ldk,
                               p.tpb, p.pos, 1e-6f, p.wb, STREAM);
}

// ---- drn_patchify_concat / drn_unpatchify
struct Pf { bool x = 1, cond = 1, out = 1; int B = 1, Cx = 16, Cc = 16, mask = 1, Tl = 2, Hl = 16, Wl = 16, pt = 1, ps = 2; int64_t ldo = 192; };
int pf(const Pf& p) {
    const int64_t plane = (int64_t)p.Tl * p.Hl * p.Wl;
    const int64_t rows = p.pt > 0 && p.ps > 0 ? (int64_t)p.B * (p.Tl / p.pt) * (p.Hl / p.ps) * (p.Wl / p.ps) : 0;
    return drn_patchify_concat(p.x ? A("x", p.B * p.Cx * plane * 2) : 0, p.cond ? A("cond", p.B * p.Cc * plane * 2) : 0,
                               p.out ? A("out", rows * p.ldo * 2) : 0, p.B, p.Cx, p.Cc, p.mask, p.Tl, p.Hl, p.Wl, p.pt, p.ps, p.ldo, STREAM);
}
struct Up { bool y = 1, out = 1; int B = 1, C = 16, Tp = 2, Hp = 8, Wp = 8, pt = 1, ps = 2; int64_t ldy = 128; };
int up(const Up& p) {
    const int64_t rows = (int64_t)p.B * p.Tp * p.Hp * p.Wp;
    return drn_unpatchify(p.y ? A("y", rows * p.ldy * 2) : 0, p.ldy, p.out ? A("out", rows * p.C * p.pt * p.ps * p.ps * 2) : 0, p.B, p.C,
                          p.Tp, p.Hp, p.Wp, p.pt, p.ps, STREAM);
}

// ---- the EDM sampler's three
struct Ew { bool a = 1, b = 1, o = 1; int64_t n = 100001; };
int edm_scale(const Ew& p) { return drn_edm_scale_input(p.a ? A("x", p.n * 2) : 0, p.o ? A("out", p.n * 2) : 0, p.n, 0.5f, STREAM); }
int edm_step(const Ew& p) {
    return drn_edm_step(p.a ? A("model_out", p.n * 2) : 0, p.b ? A("sample", p.n * 2) : 0, p.o ? A("out", p.n * 2) : 0, p.n, 0.1f, 0.9f, 2.f,
                        -0.5f, STREAM);
}
int cfg(const Ew& p) {
    return drn_cfg_combine(p.a ? A("cond", p.n * 2) : 0, p.b ? A("uncond", p.n * 2) : 0, p.o ? A("out", p.n * 2) : 0, p.n, 3.f, STREAM);
}

// ---- drn_sampler_step_2m
struct Sm { bool cond = 1, unc = 1, x = 1, hin = 1, hout = 1, xout = 1, sc = 1; int copies = 2; int64_t n = 100001; float b0 = -0.25f;
            int bf_mis = 0, fp_mis = 0; };
int sm(const Sm& p) {
    return drn_sampler_step_2m(p.cond ? A("cond", p.n * 2, p.bf_mis) : 0, p.unc ? A("uncond", p.n * 2) : 0, 3.f, p.x ? A("x", p.n * 2) : 0,
                               p.hin ? (const float*)A("hist_in", p.n * 4, p.fp_mis) : 0, p.hout ? (float*)A("hist_out", p.n * 4) : 0,
                               p.xout ? A("x_out", p.n * 2) : 0, p.sc ? A("scaled_out", (p.copies > 0 ? p.copies : 1) * p.n * 2) : 0,
                               p.copies, p.n, 0.1f, 0.9f, 0.5f, 0.75f, p.b0, 0.3f, STREAM);
}

// ---- step cache
struct Sp { bool x = 1, ref = 1, stats = 1, ws = 1; int B = 2; int64_t n = 256 * 4096 + 8; int64_t ws_short = 0; int x_mis = 0, st_mis = 0, ws_mis = 0; };
int sp(const Sp& p) {
    const int64_t need = drn_step_cache_workspace_bytes(p.B, p.n) - p.ws_short;
    return drn_step_cache_probe(p.x ? A("x", p.B * p.n * 2, p.x_mis) : 0, p.ref ? A("ref", p.B * p.n * 2) : 0,
                                p.stats ? A("stats", p.B * 16, p.st_mis) : 0, p.ws ? A("workspace", need, p.ws_mis) : 0, need, p.B, p.n,
                                STREAM);
}
struct Sr { bool a = 1, b = 1, r = 1; int64_t n = 1000003; int mis = 0; };
int sres(const Sr& p) {
    return drn_step_cache_residual(p.a ? A("x", p.n * 2, p.mis) : 0, p.b ? A("ref", p.n * 2) : 0, p.r ? A("r", p.n * 2) : 0, p.n, STREAM);
}
int sapp(const Sr& p) { return drn_step_cache_apply(p.a ? A("x", p.n * 2, p.mis) : 0, p.b ? A("r", p.n * 2) : 0, p.n, STREAM); }

// ---- drn_gemv_bf16
struct Gv { bool x = 1, w = 1, y = 1, add = 1, mul = 1; int64_t N = 4096, K = 4096; int groups = 3, batch = 2; int64_t xg = 0, xb = 4096,
            wg = 4096ll * 4096; int act = DRN_ACT_SILU; };
int gv(const Gv& p) {
    const int64_t yn = (int64_t)p.groups * p.batch * p.N * 2;
    return drn_gemv_bf16(p.x ? A("x", ((p.groups - 1) * p.xg + (p.batch - 1) * p.xb + p.K) * 2) : 0,
                         p.w ? A("W", ((p.groups - 1) * p.wg + p.N * p.K) * 2) : 0, p.y ? A("y", yn) : 0, p.N, p.K, p.groups, p.batch, p.xg,
                         p.xb, p.wg, p.batch * p.N, p.N, p.add ? A("add", yn) : 0, p.batch * p.N, p.N, p.mul ? A("mul", yn) : 0,
                         p.batch * p.N, p.N, p.act, STREAM);
}

// ---- drn_mx_quant_bf16
struct Mq { bool x = 1, q = 1, s = 1; int64_t M = 300, K = 4096, ldx = 4096; int x_mis = 0, q_mis = 0; };
int mq(const Mq& p) {
    return drn_mx_quant_bf16(p.x ? A("X", p.M * p.ldx * 2, p.x_mis) : 0, p.M, p.K, p.ldx, p.q ? A("Q", p.M * p.K, p.q_mis) : 0,
                             p.s ? A("scales", p.M * p.K / 32) : 0, STREAM);
}

}  // namespace

void family_elementwise() {
    entry<Rms>("drn_rmsnorm", rms,
               {CH(Rms, "null x", p.x = 0), CH(Rms, "null w", p.w = 0), CH(Rms, "null y", p.y = 0), CH(Rms, "rows < 0", p.rows = -1),
                CH(Rms, "D == 0", p.D = 0), CH(Rms, "D % 8", p.D = 4100),
                CH(Rms, "2^33 - 3 rows: 2^31 workgroups", (p.rows = 8 * G - 3, p.D = 8)), CH(Rms, "D == 2^31", (p.rows = 1, p.D = 2 * G))},
               {CH(Rms, "rows == 0", p.rows = 0), CH(Rms, "9e8 rows of 128", (p.rows = 900000000, p.D = 128)),
                CH(Rms, "2^33 - 4 rows: 2^31 - 1 workgroups", (p.rows = 8 * G - 4, p.D = 8)), CH(Rms, "D == 2^31 - 8", (p.rows = 1, p.D = 2 * G - 8))},
               // D: rows x D x 2 bytes either side of 2^31 and 2^32, up to ~250 GB
               {CH(Rms, "2^31 - 8 elements", (p.rows = G / 4 - 1, p.D = 8)), CH(Rms, "2^31 elements", (p.rows = G / 4, p.D = 8)),
                CH(Rms, "2^32 elements", (p.rows = G / 2, p.D = 8)), CH(Rms, "2^32 + 8 elements", (p.rows = G / 2 + 1, p.D = 8)),
                CH(Rms, "2^33 rows of 8 (128 GiB)", (p.rows = 8 * G, p.D = 8)), CH(Rms, "15e9 rows of 8 (240 GB)", (p.rows = 15000000000ll, p.D = 8))});

    const std::vector<Change<Ln>> ln_ref = {CH(Ln, "null x", p.x = 0), CH(Ln, "null shift", p.shift = 0), CH(Ln, "null scale", p.scale = 0),
                                            CH(Ln, "rows < 0", p.rows = -1), CH(Ln, "D == 0", p.D = 0), CH(Ln, "D % 8", p.D = 4100),
                                            CH(Ln, "D > 8192", p.D = 8200), CH(Ln, "rows_per_batch == 0", p.rpb = 0),
                                            CH(Ln, "2^33 - 3 rows: 2^31 workgroups", (p.rows = 8 * G - 3, p.D = 32, p.rpb = G))};
    const std::vector<Change<Ln>> ln_ok = {CH(Ln, "rows == 0", p.rows = 0), CH(Ln, "2^33 - 4 rows: 2^31 - 1 workgroups", (p.rows = 8 * G - 4, p.D = 32, p.rpb = G)), CH(Ln, "no add_vec", p.add = 0),
                                           CH(Ln, "D 256, 18432 rows", (p.D = 256, p.rows = 18432, p.rpb = 18432)),
                                           CH(Ln, "D 8192, 5000 rows", (p.D = 8192, p.rows = 5000, p.rpb = 5000))};
    const std::vector<Change<Ln>> ln_big = {CH(Ln, "2^31 - 1 rows of 32", (p.rows = 2 * G - 1, p.D = 32, p.rpb = G)),
                                            CH(Ln, "2^31 rows of 32", (p.rows = 2 * G, p.D = 32, p.rpb = G)),
                                            CH(Ln, "2^32 rows of 32 (256 GiB)", (p.rows = 4 * G, p.D = 32, p.rpb = G)),
                                            CH(Ln, "2^31 rows of 2048, no add", (p.rows = 2 * G / 64, p.D = 2048, p.rpb = G, p.add = 0)),
                                            CH(Ln, "2^33 + 4 rows of 32", (p.rows = 8 * G + 4, p.D = 32, p.rpb = G)),
                                            CH(Ln, "2^34 + 4 rows of 32", (p.rows = 16 * G + 4, p.D = 32, p.rpb = G))};
    {
        auto r = ln_ref;
        r.push_back(CH(Ln, "null h", p.h = 0));
        entry<Ln>("drn_ln_modulate", ln, r, ln_ok, ln_big);
        r = ln_ref;
        r.push_back(CH(Ln, "null hq", p.hq = 0));
        r.push_back(CH(Ln, "null hs", p.hs = 0));
        r.push_back(CH(Ln, "D % 32", p.D = 4104));
        r.push_back(CH(Ln, "hq off 8 bytes", p.hq_mis = 4));
        auto ok = ln_ok;
        ok.push_back(CH(Ln, "null h (MX only)", p.h = 0));
        entry<Ln>("drn_ln_modulate_mx", ln_mx, r, ok, ln_big);
    }

    const std::vector<Change<Sk>> sk_ref = {
        CH(Sk, "null partials", p.part = 0), CH(Sk, "null x", p.x = 0), CH(Sk, "null gate", p.gate = 0), CH(Sk, "null shift", p.shift = 0),
        CH(Sk, "null scale", p.scale = 0), CH(Sk, "splits == 0", p.splits = 0), CH(Sk, "rows < 0", p.rows = -1),
        CH(Sk, "rows == 2^31", (p.rows = 2 * G, p.D = 1032, p.splits = 1)), CH(Sk, "D == 1024", p.D = 1024), CH(Sk, "D % 8", p.D = 4100),
        CH(Sk, "D > 8192", p.D = 8200), CH(Sk, "rows_per_batch == 0", p.rpb = 0), CH(Sk, "partials off 16 bytes", p.part_mis = 8)};
    const std::vector<Change<Sk>> sk_ok = {CH(Sk, "rows == 0", p.rows = 0), CH(Sk, "no add_vec", p.add = 0),
                                           CH(Sk, "D 1056", p.D = 1056), CH(Sk, "D 8192, 1024 rows", (p.D = 8192, p.rows = 1024)),
                                           CH(Sk, "2^31 - 1 rows of 1056, 1 split", (p.rows = 2 * G - 1, p.D = 1056, p.splits = 1))};
    {
        auto r = sk_ref;
        r.push_back(CH(Sk, "null h", p.h = 0));
        entry<Sk>("drn_splitk_gate_res_ln_modulate", sk, r, sk_ok);
        r = sk_ref;
        r.push_back(CH(Sk, "null hq", p.hq = 0));
        r.push_back(CH(Sk, "null hs", p.hs = 0));
        r.push_back(CH(Sk, "D % 32", p.D = 4104));
        r.push_back(CH(Sk, "hq off 8 bytes", p.hq_mis = 4));
        auto ok = sk_ok;
        ok.push_back(CH(Sk, "null h (MX only)", p.h = 0));
        entry<Sk>("drn_splitk_gate_res_ln_modulate_mx", sk_mx, r, ok);
    }

    entry<Bc>("drn_bcast_add", bc,
              {CH(Bc, "null x", p.x = 0), CH(Bc, "null vec", p.v = 0), CH(Bc, "rows < 0", p.rows = -1), CH(Bc, "D == 0", p.D = 0),
               CH(Bc, "D % 8", p.D = 4100), CH(Bc, "rows_per_batch == 0", p.rpb = 0)},
              {CH(Bc, "rows == 0", p.rows = 0)},
              {CH(Bc, "2^31 - 8 elements", (p.rows = G / 4 - 1, p.D = 8, p.rpb = G)), CH(Bc, "2^32 elements", (p.rows = G / 2, p.D = 8, p.rpb = G)),
               CH(Bc, "2^37 elements (256 GiB)", (p.rows = 32 * G, p.D = 4096, p.rpb = G))});

    entry<Pm>("drn_permute_021", pm,
              {CH(Pm, "null x", p.x = 0), CH(Pm, "null y", p.y = 0), CH(Pm, "y == x", p.same = 1), CH(Pm, "A < 0", p.a = -1),
               CH(Pm, "B < 0", p.b = -1), CH(Pm, "C == 0", p.c = 0), CH(Pm, "C % 8", p.c = 516), CH(Pm, "x off 16 bytes", p.mis = 8), CH(Pm, "y off 16 bytes", p.y_mis = 8)},
              {CH(Pm, "A == 0", p.a = 0), CH(Pm, "B == 0", p.b = 0)},
              {CH(Pm, "2^31 elements", (p.a = G / 256, p.b = 8, p.c = 64)), CH(Pm, "2^32 + 512 elements", (p.a = G / 128 + 1, p.b = 8, p.c = 64)),
               CH(Pm, "2^36 elements (128 GiB)", (p.a = G / 8, p.b = 8, p.c = 64))});

    const std::vector<Change<Qk>> qk_ref = {
        CH(Qk, "neither q nor k", (p.q = 0, p.k = 0)), CH(Qk, "q without wq", p.wq = 0), CH(Qk, "k without wk", p.wk = 0),
        CH(Qk, "tokens < 0", p.tokens = -1), CH(Qk, "heads == 0", p.heads = 0), CH(Qk, "ldq % 8", p.ldq = 3 * 2048 + 4),
        CH(Qk, "ldk % 8", p.ldk = 3 * 2048 + 4), CH(Qk, "tokens_per_batch == 0", p.tpb = 0), CH(Qk, "cos without sin", p.sin = 0),
        CH(Qk, "sin without cos", p.cos = 0)};
    const std::vector<Change<Qk>> qk_ok = {CH(Qk, "tokens == 0", p.tokens = 0), CH(Qk, "k only", (p.q = 0, p.wq = 0)),
                                           CH(Qk, "q only", (p.k = 0, p.wk = 0)), CH(Qk, "no RoPE", (p.cos = 0, p.sin = 0)),
                                           CH(Qk, "18432 tokens, 32 heads", (p.tokens = 18432, p.heads = 32, p.ldq = p.ldk = 3 * 4096, p.tpb = 18432)),
                                           CH(Qk, "3 heads, pos_offset", (p.heads = 3, p.pos = 77))};
    entry<Qk>("drn_qk_norm_rope", qk, qk_ref, qk_ok,
              {CH(Qk, "2^31 elements in q|k|v rows", (p.tokens = G / 192, p.heads = 1, p.ldq = p.ldk = 384, p.tpb = 4096)),
               CH(Qk, "2^33 elements", (p.tokens = G / 48, p.heads = 1, p.ldq = p.ldk = 384, p.tpb = 4096)),
               CH(Qk, "2^36 elements (128 GiB)", (p.tokens = G / 6, p.heads = 1, p.ldq = p.ldk = 384, p.tpb = 4096))});
    {
        auto r = qk_ref;
        r.push_back(CH(Qk, "q without qq", p.qq = 0));
        r.push_back(CH(Qk, "q without qs", p.qs = 0));
        r.push_back(CH(Qk, "k without kq", p.kq = 0));
        r.push_back(CH(Qk, "k without ks", p.ks = 0));
        r.push_back(CH(Qk, "write_bf16 == 2", p.wb = 2));
        r.push_back(CH(Qk, "q off 16 bytes", p.q_mis = 8));
        r.push_back(CH(Qk, "qq off 8 bytes", p.qq_mis = 4));
        r.push_back(CH(Qk, "k alone off 16 bytes", p.k_mis = 8));
        r.push_back(CH(Qk, "kq off 8 bytes", p.kq_mis = 4));
        r.push_back(CH(Qk, "q alone off 16 bytes (k only moved back)", (p.q_mis = 8, p.k_mis = -8)));
        auto ok = qk_ok;
        ok[1] = CH(Qk, "k only", (p.q = 0, p.wq = 0, p.qq = 0, p.qs = 0));
        ok[2] = CH(Qk, "q only", (p.k = 0, p.wk = 0, p.kq = 0, p.ks = 0));
        ok.push_back(CH(Qk, "write_bf16 1", p.wb = 1));
        entry<Qk>("drn_qk_norm_rope_mx", qk_mx, r, ok);
    }

    entry<Pf>("drn_patchify_concat", pf,
              {CH(Pf, "null x", p.x = 0), CH(Pf, "null out", p.out = 0), CH(Pf, "B == 0", p.B = 0), CH(Pf, "Cx == 0", p.Cx = 0),
               CH(Pf, "Cc < 0", p.Cc = -1), CH(Pf, "Cc without cond", p.cond = 0), CH(Pf, "pt == 0", p.pt = 0), CH(Pf, "ps == 0", p.ps = 0),
               CH(Pf, "Tl % pt", (p.Tl = 3, p.pt = 2)), CH(Pf, "Hl % ps", p.Hl = 15), CH(Pf, "Wl % ps", p.Wl = 15), CH(Pf, "ldo short", p.ldo = 128),
               CH(Pf, "Tl == 0", p.Tl = 0), CH(Pf, "Hl == 0", p.Hl = 0), CH(Pf, "Wl < 0", p.Wl = -2)},
              {CH(Pf, "no cond", (p.Cc = 0, p.cond = 0)), CH(Pf, "no mask", p.mask = 0),
               CH(Pf, "the model's grid: 18432 tokens", (p.Tl = 8, p.Hl = 96, p.Wl = 96))},
              {CH(Pf, "output past 2^31 elements", (p.B = 16, p.Tl = 64, p.Hl = 512, p.Wl = 512)),
               CH(Pf, "inputs past 2^32 elements", (p.B = 64, p.Tl = 128, p.Hl = 512, p.Wl = 512, p.Cx = 64, p.Cc = 0, p.cond = 0, p.ldo = 264))});

    entry<Up>("drn_unpatchify", up,
              {CH(Up, "null y", p.y = 0), CH(Up, "null out", p.out = 0), CH(Up, "B == 0", p.B = 0), CH(Up, "C == 0", p.C = 0),
               CH(Up, "Tp == 0", p.Tp = 0), CH(Up, "Hp == 0", p.Hp = 0), CH(Up, "Wp == 0", p.Wp = 0), CH(Up, "pt == 0", p.pt = 0),
               CH(Up, "ps == 0", p.ps = 0), CH(Up, "ldy short", p.ldy = 56)},
              {CH(Up, "the model's grid", (p.Tp = 8, p.Hp = 48, p.Wp = 48))},
              {CH(Up, "output past 2^31 elements", (p.B = 16, p.Tp = 64, p.Hp = 256, p.Wp = 256)),
               CH(Up, "output past 2^33 elements", (p.B = 64, p.Tp = 128, p.Hp = 512, p.Wp = 256))});

    const std::vector<Change<Ew>> ew_big = {CH(Ew, "n = 2^31 - 1", p.n = 2 * G - 1), CH(Ew, "n = 2^31", p.n = 2 * G), CH(Ew, "n = 2^32 + 1", p.n = 4 * G + 1),
                                            CH(Ew, "n = 2^35 (64 GiB each)", p.n = 32 * G)};
    entry<Ew>("drn_edm_scale_input", edm_scale, {CH(Ew, "null x", p.a = 0), CH(Ew, "null out", p.o = 0), CH(Ew, "n < 0", p.n = -1)},
              {CH(Ew, "n == 0", p.n = 0), CH(Ew, "n == 1", p.n = 1)}, ew_big);
    entry<Ew>("drn_edm_step", edm_step,
              {CH(Ew, "null model_out", p.a = 0), CH(Ew, "null sample", p.b = 0), CH(Ew, "null out", p.o = 0), CH(Ew, "n < 0", p.n = -1)},
              {CH(Ew, "n == 0", p.n = 0)}, ew_big);
    entry<Ew>("drn_cfg_combine", cfg,
              {CH(Ew, "null cond", p.a = 0), CH(Ew, "null uncond", p.b = 0), CH(Ew, "null out", p.o = 0), CH(Ew, "n < 0", p.n = -1)},
              {CH(Ew, "n == 0", p.n = 0)}, ew_big);

    entry<Sm>("drn_sampler_step_2m", sm,
              {CH(Sm, "null cond", p.cond = 0), CH(Sm, "null x", p.x = 0), CH(Sm, "null hist_out", p.hout = 0), CH(Sm, "null x_out", p.xout = 0),
               CH(Sm, "copies 0 with scaled_out", p.copies = 0), CH(Sm, "copies 3 with scaled_out", p.copies = 3), CH(Sm, "n < 0", p.n = -1),
               CH(Sm, "no hist_in with b0 != 0", p.hin = 0), CH(Sm, "bf16 pointer off 2 bytes", p.bf_mis = 1),
               CH(Sm, "history off 4 bytes", p.fp_mis = 2), CH(Sm, "uncond off 2 bytes", off("uncond", 1)), CH(Sm, "x off 2 bytes", off("x", 1)),
               CH(Sm, "x_out off 2 bytes", off("x_out", 1)), CH(Sm, "scaled_out off 2 bytes", off("scaled_out", 1)), CH(Sm, "hist_out off 4 bytes", off("hist_out", 2))},
              {CH(Sm, "n == 0", p.n = 0), CH(Sm, "no CFG", (p.unc = 0, p.copies = 1)), CH(Sm, "first step: no history", (p.hin = 0, p.b0 = 0.f)),
               CH(Sm, "last step: no scaled_out, copies ignored", (p.sc = 0, p.copies = 7)), CH(Sm, "unaligned by 2 bytes", p.bf_mis = 2),
               CH(Sm, "n % 8 == 0", p.n = 1 << 20)},
              {CH(Sm, "n = 2^31 - 1", p.n = 2 * G - 1), CH(Sm, "n = 2^31", p.n = 2 * G), CH(Sm, "n = 2^32 + 8", p.n = 4 * G + 8),
               CH(Sm, "n = 2^34 (~250 GB of operands)", p.n = 16 * G)});

    entry<Sp>("drn_step_cache_probe", sp,
              {CH(Sp, "null x", p.x = 0), CH(Sp, "null ref", p.ref = 0), CH(Sp, "null stats", p.stats = 0), CH(Sp, "null workspace", p.ws = 0),
               CH(Sp, "workspace one byte short", p.ws_short = 1), CH(Sp, "B == 0", p.B = 0), CH(Sp, "n == 0", p.n = 0),
               CH(Sp, "x off 2 bytes", p.x_mis = 1), CH(Sp, "ref off 2 bytes", off("ref", 1)), CH(Sp, "stats off 8 bytes", p.st_mis = 4), CH(Sp, "workspace off 8 bytes", p.ws_mis = 4)},
              {CH(Sp, "n == 1", p.n = 1), CH(Sp, "x off the 16-byte grid", p.x_mis = 2), CH(Sp, "the model: 18432 x 4096", (p.n = 18432ll * 4096, p.B = 2))},
              {CH(Sp, "n = 2^31 - 8", (p.n = 2 * G - 8, p.B = 1)), CH(Sp, "n = 2^31", (p.n = 2 * G, p.B = 1)), CH(Sp, "n = 2^32 + 8", (p.n = 4 * G + 8, p.B = 1)),
               CH(Sp, "B 16 x n 2^31 (128 GiB)", (p.n = 2 * G, p.B = 16)), CH(Sp, "B 65536 x n 2^19", (p.n = 1 << 19, p.B = 65536)),
               CH(Sp, "n = 2^35", (p.n = 32 * G, p.B = 1))});
    const std::vector<Change<Sr>> sr_big = {CH(Sr, "n = 2^31 - 1", p.n = 2 * G - 1), CH(Sr, "n = 2^31", p.n = 2 * G), CH(Sr, "n = 2^32 + 3", p.n = 4 * G + 3),
                                            CH(Sr, "n = 2^35", p.n = 32 * G)};
    entry<Sr>("drn_step_cache_residual", sres,
              {CH(Sr, "null x", p.a = 0), CH(Sr, "null ref", p.b = 0), CH(Sr, "null r", p.r = 0), CH(Sr, "n == 0", p.n = 0),
               CH(Sr, "x off 2 bytes", p.mis = 1), CH(Sr, "ref off 2 bytes", off("ref", 1)), CH(Sr, "r off 2 bytes", off("r", 1))},
              {CH(Sr, "n == 1", p.n = 1), CH(Sr, "x off the 16-byte grid", p.mis = 6)}, sr_big);
    entry<Sr>("drn_step_cache_apply", sapp,
              {CH(Sr, "null x", p.a = 0), CH(Sr, "null r", p.b = 0), CH(Sr, "n == 0", p.n = 0), CH(Sr, "x off 2 bytes", p.mis = 1), CH(Sr, "r off 2 bytes", off("r", 1))},
              {CH(Sr, "n == 1", p.n = 1)}, sr_big);

    entry<Gv>("drn_gemv_bf16", gv,
              {CH(Gv, "null x", p.x = 0), CH(Gv, "null W", p.w = 0), CH(Gv, "null y", p.y = 0), CH(Gv, "N == 0", p.N = 0), CH(Gv, "K == 0", p.K = 0),
               CH(Gv, "K % 8", p.K = 4100), CH(Gv, "groups == 0", p.groups = 0), CH(Gv, "batch == 0", p.batch = 0),
               CH(Gv, "groups > 65535", p.groups = 65536), CH(Gv, "batch > 65535", p.batch = 65536), CH(Gv, "x_gstride % 8", p.xg = 4),
               CH(Gv, "x_bstride % 8", p.xb = 4100), CH(Gv, "w_gstride % 8", p.wg = 4096ll * 4096 + 4), CH(Gv, "act == 2", p.act = 2)},
              {CH(Gv, "no add, no mul", (p.add = 0, p.mul = 0)), CH(Gv, "one group, one batch", (p.groups = 1, p.batch = 1)),
               CH(Gv, "AdaLN: 84 sites x 3", (p.groups = 252, p.N = 4096, p.K = 256, p.wg = 4096 * 256, p.xb = 256))},
              {CH(Gv, "N = 2^31 + 4096 rows", (p.N = 2 * G + 4096, p.K = 8, p.groups = 1, p.batch = 1, p.xb = 8, p.wg = 0))});

    entry<Mq>("drn_mx_quant_bf16", mq,
              {CH(Mq, "null X", p.x = 0), CH(Mq, "null Q", p.q = 0), CH(Mq, "null scales", p.s = 0), CH(Mq, "M == 0", p.M = 0),
               CH(Mq, "K == 0", p.K = 0), CH(Mq, "K % 32", p.K = 4104), CH(Mq, "ldx < K", p.ldx = 4088), CH(Mq, "ldx % 8", (p.ldx = 4100)),
               CH(Mq, "X off 16 bytes", p.x_mis = 8), CH(Mq, "Q off 8 bytes", p.q_mis = 4), CH(Mq, "M K / 8 == 2^31", (p.M = G / 2, p.K = 32, p.ldx = 32)), CH(Mq, "M K / 8 == 2^31 - 252: idle lanes past 2^31", (p.M = G / 2 - 63, p.K = 32, p.ldx = 32))},
              {CH(Mq, "ldx > K", p.ldx = 3 * 4096), CH(Mq, "M K / 8 == 2^31 - 256", (p.M = G / 2 - 64, p.K = 32, p.ldx = 32)),
               CH(Mq, "18432 x 16384", (p.M = 18432, p.K = 16384, p.ldx = 16384))});
}

}  // namespace hw
