// host walk, the attention family: bf16 and MXFP8 attention, their split-KV forms and MX outputs, the V^T quantiser.
#include "host_walk.h"

namespace hw {
namespace {

struct At {
    bool q = 1, k = 1, v = 1, o = 1, oq = 1, os = 1, ws = 1;
    int batch = 2, heads = 16, nsplit = 4;
    int64_t Sq = 2304, Sk = 2309, ldq = 0, ldk = 0, ldv = 0, ldo = 0, bsq = -1, bsk = -1, bsv = -1, bso = -1;   // 0 / -1: tight
    float scale = 0.0883883f;
    int q_mis = 0, k_mis = 0, v_mis = 0, o_mis = 0, oq_mis = 0, os_mis = 0, ws_mis = 0;
};
struct AtArgs {
    void *q, *k, *v, *o, *oq, *os, *ws;
    int64_t ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso;
};
AtArgs at_args(const At& p, bool mx_out, bool split) {
    AtArgs a;
    const int64_t D = (int64_t)p.heads * 128;
    a.ldq = p.ldq ? p.ldq : D, a.ldk = p.ldk ? p.ldk : D, a.ldv = p.ldv ? p.ldv : D, a.ldo = p.ldo ? p.ldo : D;
    a.bsq = p.bsq >= 0 ? p.bsq : p.Sq * a.ldq, a.bsk = p.bsk >= 0 ? p.bsk : p.Sk * a.ldk, a.bsv = p.bsv >= 0 ? p.bsv : p.Sk * a.ldv;
    a.bso = p.bso >= 0 ? p.bso : p.Sq * a.ldo;
    auto span = [&](int64_t bs, int64_t S, int64_t ld) { return ((p.batch - 1) * bs + (S - 1) * ld + D) * 2; };
    a.q = p.q ? A("q", span(a.bsq, p.Sq, a.ldq), p.q_mis) : 0;
    a.k = p.k ? A("k", span(a.bsk, p.Sk, a.ldk), p.k_mis) : 0;
    a.v = p.v ? A("v", span(a.bsv, p.Sk, a.ldv), p.v_mis) : 0;
    a.o = p.o ? A("o", span(a.bso, p.Sq, a.ldo), p.o_mis) : 0;
    const int64_t rows = a.ldo > 0 ? (p.batch - 1) * (a.bso / a.ldo) + p.Sq : 0;
    a.oq = mx_out && p.oq ? A("oq", rows * D, p.oq_mis) : 0;
    a.os = mx_out && p.os ? A("os", rows * D / 32, p.os_mis) : 0;
    a.ws = split && p.ws ? A("workspace", drn_attention_splitkv_workspace_bytes(p.batch, p.heads, p.Sq, p.nsplit), p.ws_mis) : 0;
    return a;
}
int att(const At& p) {
    const AtArgs a = at_args(p, false, false);
    return drn_attention_bf16(a.q, a.k, a.v, a.o, p.batch, p.heads, p.Sq, p.Sk, a.ldq, a.ldk, a.ldv, a.ldo, a.bsq, a.bsk, a.bsv, a.bso, p.scale, STREAM);
}
int att_mx(const At& p) {
    const AtArgs a = at_args(p, true, false);
    return drn_attention_bf16_mx(a.q, a.k, a.v, a.o, a.oq, a.os, p.batch, p.heads, p.Sq, p.Sk, a.ldq, a.ldk, a.ldv, a.ldo, a.bsq, a.bsk, a.bsv, a.bso,
                                 p.scale, STREAM);
}
int att_s(const At& p) {
    const AtArgs a = at_args(p, false, true);
    return drn_attention_splitkv_bf16(a.q, a.k, a.v, a.o, p.batch, p.heads, p.Sq, p.Sk, a.ldq, a.ldk, a.ldv, a.ldo, a.bsq, a.bsk, a.bsv, a.bso, p.scale,
                                      p.nsplit, a.ws, STREAM);
}
int att_s_mx(const At& p) {
    const AtArgs a = at_args(p, true, true);
    return drn_attention_splitkv_bf16_mx(a.q, a.k, a.v, a.o, a.oq, a.os, p.batch, p.heads, p.Sq, p.Sk, a.ldq, a.ldk, a.ldv, a.ldo, a.bsq, a.bsk, a.bsv,
                                         a.bso, p.scale, p.nsplit, a.ws, STREAM);
}

// ---- MXFP8 attention
struct Am {
    bool qq = 1, qs = 1, kq = 1, ks = 1, vt = 1, vs = 1, o = 1, oq = 1, os = 1, ws = 1;
    int batch = 2, heads = 16, nsplit = 4;
    int64_t Sq = 2304, Sk = 2309, q_bs = -1, k_bs = -1, ldo = 0, bso = -1;
    float scale = 0.0883883f;
    int qq_mis = 0, qs_mis = 0, kq_mis = 0, ks_mis = 0, vt_mis = 0, vs_mis = 0, o_mis = 0, oq_mis = 0, os_mis = 0, ws_mis = 0;
};
int att_mxfp8_call(const Am& p, bool split) {
    const int64_t D = (int64_t)p.heads * 128, Skp = (p.Sk + 127) / 128 * 128;
    const int64_t q_bs = p.q_bs >= 0 ? p.q_bs : p.Sq, k_bs = p.k_bs >= 0 ? p.k_bs : p.Sk, ldo = p.ldo ? p.ldo : D, bso = p.bso >= 0 ? p.bso : p.Sq * ldo;
    const int64_t qrows = (p.batch - 1) * q_bs + p.Sq, krows = (p.batch - 1) * k_bs + p.Sk, orows = ldo > 0 ? (p.batch - 1) * (bso / ldo) + p.Sq : 0;
    void* qq = p.qq ? A("qq", qrows * D, p.qq_mis) : 0;
    void* qs = p.qs ? A("qs", qrows * D / 32, p.qs_mis) : 0;
    void* kq = p.kq ? A("kq", krows * D, p.kq_mis) : 0;
    void* ks = p.ks ? A("ks", krows * D / 32, p.ks_mis) : 0;
    void* vt = p.vt ? A("vt", p.batch * D * Skp, p.vt_mis) : 0;
    void* vs = p.vs ? A("vs", p.batch * D * Skp / 32, p.vs_mis) : 0;
    void* o = p.o ? A("o", ((p.batch - 1) * bso + (p.Sq - 1) * ldo + D) * 2, p.o_mis) : 0;
    void* oq = p.oq ? A("oq", orows * D, p.oq_mis) : 0;
    void* os = p.os ? A("os", orows * D / 32, p.os_mis) : 0;
    if (!split) return drn_attention_mxfp8(qq, qs, kq, ks, vt, vs, o, oq, os, p.batch, p.heads, p.Sq, p.Sk, q_bs, k_bs, ldo, bso, p.scale, STREAM);
    void* ws = p.ws ? A("workspace", drn_attention_splitkv_workspace_bytes(p.batch, p.heads, p.Sq, p.nsplit), p.ws_mis) : 0;
    return drn_attention_splitkv_mxfp8(qq, qs, kq, ks, vt, vs, o, oq, os, p.batch, p.heads, p.Sq, p.Sk, q_bs, k_bs, ldo, bso, p.scale, p.nsplit, ws, STREAM);
}
int am(const Am& p) { return att_mxfp8_call(p, false); }
int am_s(const Am& p) { return att_mxfp8_call(p, true); }

struct Vt { bool v = 1, vt = 1, vs = 1; int batch = 2, heads = 16; int64_t Sk = 2309, ldv = 3 * 2048, bsv = -1; int v_mis = 0, vt_mis = 0, vs_mis = 0; };
int vt(const Vt& p) {
    const int64_t D = (int64_t)p.heads * 128, Skp = (p.Sk + 127) / 128 * 128, bsv = p.bsv >= 0 ? p.bsv : p.Sk * p.ldv;
    return drn_mx_quant_vt(p.v ? A("v", ((p.batch - 1) * bsv + (p.Sk - 1) * p.ldv + D) * 2, p.v_mis) : 0, p.vt ? A("vt", p.batch * D * Skp, p.vt_mis) : 0,
                           p.vs ? A("vs", p.batch * D * Skp / 32, p.vs_mis) : 0, p.batch, p.heads, p.Sk, p.ldv, bsv, STREAM);
}

}  // namespace

void family_attention() {
    const std::vector<Change<At>> ref = {
        CH(At, "null q", p.q = 0), CH(At, "null k", p.k = 0), CH(At, "null v", p.v = 0), CH(At, "batch == 0", p.batch = 0), CH(At, "heads == 0", p.heads = 0),
        CH(At, "Sq < 0", p.Sq = -1), CH(At, "Sk == 0", p.Sk = 0), CH(At, "ldq % 8", p.ldq = 2052), CH(At, "ldk % 8", p.ldk = 2052), CH(At, "ldv % 8", p.ldv = 2052),
        CH(At, "ldo % 8", p.ldo = 2052), CH(At, "bsq % 8", p.bsq = 2304 * 2048 + 4), CH(At, "bsk % 8", p.bsk = 2309 * 2048 + 4), CH(At, "bsv % 8", p.bsv = 2309 * 2048 + 4),
        CH(At, "bso % 8", p.bso = 2304 * 2048 + 4), CH(At, "q off 16 bytes", p.q_mis = 8), CH(At, "k off 16 bytes", p.k_mis = 8), CH(At, "v off 16 bytes", p.v_mis = 8),
        CH(At, "o off 16 bytes", p.o_mis = 8), CH(At, "64 ldk 2 == 2^32", (p.ldk = 1 << 25, p.Sk = 8, p.batch = 1)), CH(At, "64 ldv 2 == 2^32", (p.ldv = 1 << 25, p.Sk = 8, p.batch = 1)),
        CH(At, "2^31 workgroups", (p.batch = 65535, p.heads = 16, p.Sq = 512 * 2049, p.Sk = 1, p.nsplit = 1))};
    const std::vector<Change<At>> mx_ref = {CH(At, "null oq", p.oq = 0), CH(At, "null os", p.os = 0), CH(At, "ldo != heads 128", p.ldo = 4096),
                                            CH(At, "bso % ldo", p.bso = 2304 * 2048 + 8), CH(At, "oq off 8 bytes", p.oq_mis = 4), CH(At, "os off 4 bytes", p.os_mis = 2),
                                            CH(At, "clips closer than Sq rows", p.bso = 2303 * 2048)};
    const std::vector<Change<At>> split_ref = {CH(At, "nsplit == 0", p.nsplit = 0), CH(At, "null workspace", p.ws = 0), CH(At, "workspace off 16 bytes", p.ws_mis = 8),
                                               CH(At, "batch > 65535 with split keys", (p.batch = 65536, p.heads = 1, p.Sq = 1, p.Sk = 300))};
    const std::vector<Change<At>> ok = {CH(At, "Sq == 0", p.Sq = 0), CH(At, "one query, one key", (p.Sq = 1, p.Sk = 1)), CH(At, "views into the fused QKV", (p.ldq = p.ldk = p.ldv = 3 * 2048, p.Sk = 2304)),
                                        CH(At, "18432 tokens, 32 heads", (p.heads = 32, p.Sq = p.Sk = 18432, p.batch = 1)), CH(At, "one head", p.heads = 1),
                                        CH(At, "64 ldk 2 just below 2^32", (p.ldk = (1 << 25) - 8, p.Sk = 8, p.batch = 1))};
    {
        auto r = ref;
        r.push_back(CH(At, "null o", p.o = 0));
        entry<At>("drn_attention_bf16", att, r, ok);
        r = ref;
        r.insert(r.end(), mx_ref.begin(), mx_ref.end());
        auto k = ok;
        k.push_back(CH(At, "no bf16 output", p.o = 0));
        entry<At>("drn_attention_bf16_mx", att_mx, r, k);
        r = ref;
        r.push_back(CH(At, "null o", p.o = 0));
        r.insert(r.end(), split_ref.begin(), split_ref.end());
        k = ok;
        k.push_back(CH(At, "nsplit 1: no workspace", (p.nsplit = 1, p.ws = 0)));
        k.push_back(CH(At, "more chunks than key tiles", (p.Sk = 100, p.nsplit = 16)));
        k.push_back(CH(At, "nsplit 64", p.nsplit = 64));
        entry<At>("drn_attention_splitkv_bf16", att_s, r, k);
        r = ref;
        r.insert(r.end(), mx_ref.begin(), mx_ref.end());
        r.insert(r.end(), split_ref.begin(), split_ref.end());
        k.push_back(CH(At, "no bf16 output", p.o = 0));
        entry<At>("drn_attention_splitkv_bf16_mx", att_s_mx, r, k);
    }
    {
        // with the 32x32x16 body selected the MX outputs do not exist: the header's refusal
        drn_attention_force_shape16(0);
        if (!list_only) {
            expect_refusal("drn_attention_bf16_mx: the 32x32x16 body selected", [] { return att_mx(At()); });
            expect_refusal("drn_attention_splitkv_bf16_mx: the 32x32x16 body selected", [] { return att_s_mx(At()); });
            expect_ok("drn_attention_bf16: the 32x32x16 body", [] { return att(At()); });
            expect_ok("drn_attention_splitkv_bf16: the 32x32x16 body", [] { return att_s(At()); });
        }
        drn_attention_force_shape16(-1);
    }

    const std::vector<Change<Am>> am_ref = {
        CH(Am, "null qq", p.qq = 0), CH(Am, "null qs", p.qs = 0), CH(Am, "null kq", p.kq = 0), CH(Am, "null ks", p.ks = 0), CH(Am, "null vt", p.vt = 0), CH(Am, "null vs", p.vs = 0),
        CH(Am, "neither o nor oq", (p.o = 0, p.oq = 0, p.os = 0)), CH(Am, "oq without os", p.os = 0), CH(Am, "batch == 0", p.batch = 0), CH(Am, "heads == 0", p.heads = 0),
        CH(Am, "Sq < 0", p.Sq = -1), CH(Am, "Sk == 0", p.Sk = 0), CH(Am, "scale == 0", p.scale = 0.f), CH(Am, "scale < 0", p.scale = -1.f), CH(Am, "q_bs < Sq", p.q_bs = 2303),
        CH(Am, "k_bs < Sk", p.k_bs = 2308), CH(Am, "qq off 16 bytes", p.qq_mis = 8), CH(Am, "kq off 16 bytes", p.kq_mis = 8), CH(Am, "vt off 16 bytes", p.vt_mis = 8),
        CH(Am, "qs off 4 bytes", p.qs_mis = 2), CH(Am, "ks off 4 bytes", p.ks_mis = 2), CH(Am, "vs off 4 bytes", p.vs_mis = 2), CH(Am, "o off 16 bytes", p.o_mis = 8),
        CH(Am, "oq off 8 bytes", p.oq_mis = 4), CH(Am, "os off 4 bytes", p.os_mis = 2), CH(Am, "ldo % 8", p.ldo = 2052), CH(Am, "bso % 8", (p.bso = 2304 * 2048 + 4, p.oq = 0, p.os = 0)),
        CH(Am, "ldo < heads 128", (p.ldo = 1024, p.oq = 0, p.os = 0)), CH(Am, "oq with ldo != heads 128", p.ldo = 4096), CH(Am, "oq with bso % ldo", p.bso = 2304 * 2048 + 8)};
    const std::vector<Change<Am>> am_ok = {CH(Am, "Sq == 0", p.Sq = 0), CH(Am, "one query, one key", (p.Sq = 1, p.Sk = 1)), CH(Am, "bf16 output only", (p.oq = 0, p.os = 0)),
                                           CH(Am, "MX output only", p.o = 0), CH(Am, "18432 tokens, 32 heads", (p.heads = 32, p.Sq = p.Sk = 18432, p.batch = 1)),
                                           CH(Am, "strided bf16 output", (p.ldo = 4096, p.oq = 0, p.os = 0))};
    entry<Am>("drn_attention_mxfp8", am, am_ref, am_ok);
    {
        auto r = am_ref;
        r.push_back(CH(Am, "nsplit == 0", p.nsplit = 0));
        r.push_back(CH(Am, "null workspace", p.ws = 0));
        r.push_back(CH(Am, "workspace off 16 bytes", p.ws_mis = 8));
        auto k = am_ok;
        k.push_back(CH(Am, "nsplit 1: no workspace", (p.nsplit = 1, p.ws = 0)));
        k.push_back(CH(Am, "more chunks than key tiles", (p.Sk = 100, p.nsplit = 16)));
        entry<Am>("drn_attention_splitkv_mxfp8", am_s, r, k);
    }
    entry<Vt>("drn_mx_quant_vt", vt,
              {CH(Vt, "null v", p.v = 0), CH(Vt, "null vt", p.vt = 0), CH(Vt, "null vs", p.vs = 0), CH(Vt, "batch == 0", p.batch = 0), CH(Vt, "batch > 65535", (p.batch = 65536, p.Sk = 4, p.heads = 1, p.ldv = 128)),
               CH(Vt, "heads == 0", p.heads = 0), CH(Vt, "heads > 65535", (p.heads = 65536, p.Sk = 4, p.batch = 1, p.ldv = 65536 * 128)), CH(Vt, "Sk == 0", p.Sk = 0), CH(Vt, "ldv < heads 128", p.ldv = 1024),
               CH(Vt, "ldv % 8", p.ldv = 2052), CH(Vt, "bsv % 8", p.bsv = 2309 * 6144 + 4), CH(Vt, "v off 16 bytes", p.v_mis = 8), CH(Vt, "vt off 16 bytes", p.vt_mis = 8), CH(Vt, "vs off 4 bytes", p.vs_mis = 2)},
              {CH(Vt, "one key", p.Sk = 1), CH(Vt, "bsv 0: one clip shared", p.bsv = 0), CH(Vt, "18432 keys, 32 heads", (p.Sk = 18432, p.heads = 32, p.ldv = 3 * 4096)),
               CH(Vt, "2^31 keys, one head (512 GiB: the grid only)", (p.Sk = 1ll << 31, p.heads = 1, p.batch = 1, p.ldv = 128))});
}

}  // namespace hw
