// host walk, the GEMM family: the bf16 and MXFP8 products (sections A and D), and section B: the launches of drn_gemm_bf16,
// _blocked and _splitk are the records of drn_gemm_plan_describe - same kernels, same order, A and C advanced to the record's row.
#include <string.h>

#include <algorithm>

#include "host_walk.h"

namespace hw {
namespace {

const int64_t G = 1ll << 30;

struct Gm {
    bool A = 1, W = 1, C = 1, gate = 1, res = 1, ws = 1;
    int64_t M = 2304, N = 4096, K = 4096, lda = 0, ldw = 0, ldc = 0, ldr = 0, rpb = 2304;   // ld 0: the tight stride
    int epi = DRN_EPI_GATE_RES, splits = 4;
    int64_t a_cols = 512, a_stride = -1, c_cols = 512, c_stride = -1;                       // blocked entry only; stride -1: planes of M rows
    int A_mis = 0, W_mis = 0, C_mis = 0, R_mis = 0, ws_mis = 0;
};
struct GmArgs {
    void *A, *W, *C, *gate, *res, *ws;
    int64_t lda, ldw, ldc, ldr, a_stride, c_stride;
};
GmArgs gm_args(const Gm& p, bool blocked, bool with_ws) {
    GmArgs a;
    const int64_t ac = blocked ? p.a_cols : 0, cc = blocked ? p.c_cols : 0;
    a.lda = p.lda ? p.lda : (ac ? ac : p.K);
    a.ldw = p.ldw ? p.ldw : p.K;
    a.ldc = p.ldc ? p.ldc : (cc ? cc : p.N);
    a.ldr = p.ldr ? p.ldr : p.N + 64;                                 // ldr != ldc
    a.a_stride = p.a_stride >= 0 ? p.a_stride : p.M * a.lda;
    a.c_stride = p.c_stride >= 0 ? p.c_stride : p.M * a.ldc;
    const int64_t a_el = ac > 0 ? (p.K / ac - 1) * a.a_stride + (p.M - 1) * a.lda + ac : (p.M - 1) * a.lda + p.K;
    const int64_t c_el = cc > 0 ? (p.N / cc - 1) * a.c_stride + (p.M - 1) * a.ldc + cc : (p.M - 1) * a.ldc + p.N;
    const int64_t clips = p.rpb > 0 ? (p.M + p.rpb - 1) / p.rpb : 1;
    a.A = p.A ? A("A", a_el * 2, p.A_mis) : 0;
    a.W = p.W ? A("W", ((p.N - 1) * a.ldw + p.K) * 2, p.W_mis) : 0;
    a.C = p.C ? A("C", c_el * 2, p.C_mis) : 0;
    a.gate = p.gate ? A("gate", clips * p.N * 2) : 0;
    a.res = p.res ? A("residual", ((p.M - 1) * a.ldr + p.N) * 2, p.R_mis) : 0;
    a.ws = with_ws && p.ws ? A("workspace", drn_gemm_splitk_workspace_bytes(p.M, p.N, p.splits), p.ws_mis) : 0;
    return a;
}
int gemm(const Gm& p) {
    const GmArgs a = gm_args(p, false, false);
    return drn_gemm_bf16(a.A, a.W, a.C, p.M, p.N, p.K, a.lda, a.ldw, a.ldc, p.epi, a.gate, a.res, a.ldr, p.rpb, STREAM);
}
int gemm_blocked(const Gm& p) {
    const GmArgs a = gm_args(p, true, false);
    return drn_gemm_bf16_blocked(a.A, a.W, a.C, p.M, p.N, p.K, a.lda, a.ldw, a.ldc, p.epi, a.gate, a.res, a.ldr, p.rpb, p.a_cols, a.a_stride,
                                 p.c_cols, a.c_stride, STREAM);
}
struct GmS : Gm { GmS() { M = 256, rpb = 256; } };
int gemm_splitk(const GmS& p) {
    const GmArgs a = gm_args(p, false, true);
    return drn_gemm_bf16_splitk(a.A, a.W, a.C, p.M, p.N, p.K, a.lda, a.ldw, a.ldc, p.epi, a.gate, a.res, a.ldr, p.rpb, p.splits, a.ws, STREAM);
}
int gemm_partials(const GmS& p) {
    const GmArgs a = gm_args(p, false, true);
    return drn_gemm_bf16_splitk_partials(a.A, a.W, p.M, p.N, p.K, a.lda, a.ldw, p.rpb, p.splits, a.ws, STREAM);
}
struct GmF : Gm { GmF() { M = 9216, N = 9216, K = 512; } };
int gemm_f32(const GmF& p) {
    const int64_t lda = p.lda ? p.lda : p.K, ldw = p.ldw ? p.ldw : p.K;
    return drn_gemm_bf16_f32out(p.A ? A("A", ((p.M - 1) * lda + p.K) * 2, p.A_mis) : 0, p.W ? A("W", ((p.N - 1) * ldw + p.K) * 2, p.W_mis) : 0,
                                p.C ? (float*)A("C", p.M * p.N * 4, p.C_mis) : 0, p.M, p.N, p.K, lda, ldw, STREAM);
}

// ---- MXFP8
struct Mx {
    bool A = 1, SA = 1, W = 1, SW = 1, C = 1, CS = 1, gate = 1, res = 1, ws = 1;
    int64_t M = 2304, N = 4096, K = 4096, ldc = 0, ldr = 0, rpb = 2304;
    int epi = DRN_EPI_GATE_RES, splits = 4;
    int64_t a_cols = 512, a_stride = -1, c_cols = 512, c_stride = -1;
    int A_mis = 0, SA_mis = 0, W_mis = 0, SW_mis = 0, C_mis = 0, R_mis = 0, G_mis = 0, ws_mis = 0;
};
struct MxArgs {
    void *A, *SA, *W, *SW, *C, *gate, *res, *ws;
    int64_t ldc, ldr, a_stride, c_stride;
};
MxArgs mx_args(const Mx& p, bool blocked, bool with_ws) {
    MxArgs a;
    const int64_t ac = blocked ? p.a_cols : 0, cc = blocked ? p.c_cols : 0;
    a.ldc = p.ldc ? p.ldc : (cc ? cc : p.N);
    a.ldr = p.ldr ? p.ldr : p.N + 64;
    a.a_stride = p.a_stride >= 0 ? p.a_stride : p.M * ac;
    a.c_stride = p.c_stride >= 0 ? p.c_stride : p.M * a.ldc;
    const int64_t a_by = ac > 0 ? (p.K / ac - 1) * a.a_stride + p.M * ac : p.M * p.K;
    const int64_t c_el = cc > 0 ? (p.N / cc - 1) * a.c_stride + (p.M - 1) * a.ldc + cc : (p.M - 1) * a.ldc + p.N;
    const int64_t clips = p.rpb > 0 ? (p.M + p.rpb - 1) / p.rpb : 1;
    a.A = p.A ? A("A", a_by, p.A_mis) : 0;
    a.SA = p.SA ? A("SA", a_by / 32, p.SA_mis) : 0;
    a.W = p.W ? A("W", p.N * p.K, p.W_mis) : 0;
    a.SW = p.SW ? A("SW", p.N * p.K / 32, p.SW_mis) : 0;
    a.C = p.C ? A("C", c_el * 2, p.C_mis) : 0;
    a.gate = p.gate ? A("gate", clips * p.N * 2, p.G_mis) : 0;
    a.res = p.res ? A("residual", ((p.M - 1) * a.ldr + p.N) * 2, p.R_mis) : 0;
    a.ws = with_ws && p.ws ? A("workspace", drn_gemm_splitk_workspace_bytes(p.M, p.N, p.splits), p.ws_mis) : 0;
    return a;
}
int mx(const Mx& p) {
    const MxArgs a = mx_args(p, false, false);
    return drn_gemm_mxfp8(a.A, a.SA, a.W, a.SW, a.C, p.M, p.N, p.K, a.ldc, p.epi, a.gate, a.res, a.ldr, p.rpb, STREAM);
}
int mx_blocked(const Mx& p) {
    const MxArgs a = mx_args(p, true, false);
    return drn_gemm_mxfp8_blocked(a.A, a.SA, a.W, a.SW, a.C, p.M, p.N, p.K, a.ldc, p.epi, a.gate, a.res, a.ldr, p.rpb, p.a_cols, a.a_stride, p.c_cols,
                                  a.c_stride, STREAM);
}
struct MxS : Mx { MxS() { M = 256, rpb = 256; } };
int mx_splitk(const MxS& p) {
    const MxArgs a = mx_args(p, false, true);
    return drn_gemm_mxfp8_splitk(a.A, a.SA, a.W, a.SW, a.C, p.M, p.N, p.K, a.ldc, p.epi, a.gate, a.res, a.ldr, p.rpb, p.splits, a.ws, STREAM);
}
int mx_partials(const MxS& p) {
    const MxArgs a = mx_args(p, false, true);
    return drn_gemm_mxfp8_splitk_partials(a.A, a.SA, a.W, a.SW, p.M, p.N, p.K, p.rpb, p.splits, a.ws, STREAM);
}
struct MxG : Mx { MxG() { N = 16384; } };
int mx_gelu(const MxG& p) {
    return drn_gemm_mxfp8_gelu_mx(p.A ? A("A", p.M * p.K, p.A_mis) : 0, p.SA ? A("SA", p.M * p.K / 32, p.SA_mis) : 0, p.W ? A("W", p.N * p.K, p.W_mis) : 0,
                                  p.SW ? A("SW", p.N * p.K / 32, p.SW_mis) : 0, p.C ? A("CQ", p.M * p.N, p.C_mis) : 0, p.CS ? A("CS", p.M * p.N / 32) : 0,
                                  p.M, p.N, p.K, p.rpb, STREAM);
}

// ------------------------------------------------------------------------------------------------ section B
const char* kernel_name(int64_t id) {
    switch (id) {
        case 0: return "gemm_bf16_kernel<";
        case 1: return "gemm256s_kernel<";
        case 2: return "gemm144_kernel<";
        case 5: return "gemm384_kernel<";
        case 6: return "gemm_tall_kernel<";
    }
    return "?";
}
bool is_kernel(const rec::Launch& l, int64_t id) {
    const std::string k = l.kernel;
    if (id == 1 && k.find("gemm256w_kernel(") != std::string::npos) return true;      // the weight-ring form of the 256-row slices
    return k.find(std::string("void ") + kernel_name(id)) == 0;
}

long plan_cases = 0, plan_launches = 0, plan_refusals = 0;

// one product under the current settings: the call against its description
void plan_equals_launches(const std::string& label, const Gm& p, int variant) {    // 0 plain, 1 blocked A, 2 blocked C, 3 split-K
    Gm q = p;
    if (variant == 0) q.a_cols = q.c_cols = 0;
    if (variant == 1) q.c_cols = 0;
    if (variant == 2) q.a_cols = 0;
    if (variant == 3) q.a_cols = q.c_cols = 0;
    const int splits = variant == 3 ? q.splits : 1;
    rec::reset();
    const bool blocked = variant == 1 || variant == 2;
    const GmArgs a = gm_args(q, blocked, variant == 3);
    int64_t* recs = new int64_t[4 * 64];                     // a heap block: ASan guards what describe writes
    const int n = drn_gemm_plan_describe(q.M, q.N, q.K, a.lda, a.ldw, a.ldc, a.ldr, q.epi, q.rpb, blocked ? q.a_cols : 0, blocked ? q.c_cols : 0, splits,
                                         recs, 64);
    int rc;
    if (variant == 3)
        rc = drn_gemm_bf16_splitk(a.A, a.W, a.C, q.M, q.N, q.K, a.lda, a.ldw, a.ldc, q.epi, a.gate, a.res, a.ldr, q.rpb, splits, a.ws, STREAM);
    else if (blocked)
        rc = drn_gemm_bf16_blocked(a.A, a.W, a.C, q.M, q.N, q.K, a.lda, a.ldw, a.ldc, q.epi, a.gate, a.res, a.ldr, q.rpb, q.a_cols, a.a_stride, q.c_cols,
                                   a.c_stride, STREAM);
    else
        rc = drn_gemm_bf16(a.A, a.W, a.C, q.M, q.N, q.K, a.lda, a.ldw, a.ldc, q.epi, a.gate, a.res, a.ldr, q.rpb, STREAM);
    ++plan_cases;
    const auto& L = rec::launches();
    if (n < 0 || rc == DRN_EINVAL) {
        // a refusal in one must be a refusal in the other
        if (!(n < 0 && rc == DRN_EINVAL)) fail(label + ": describe says " + std::to_string(n) + ", the call returns " + std::to_string(rc));
        if (!L.empty()) fail(label + ": refused after launching");
        ++plan_refusals;
        delete[] recs;
        return;
    }
    if (rc != DRN_OK) fail(label + ": the call returns " + std::to_string(rc));
    const std::string bad = rec::check_call();
    if (!bad.empty()) fail(label + ": " + bad);
    const size_t want = (size_t)n + (variant == 3 ? 1 : 0);                          // split-K: the slice launch, then the reduce
    if (n > 64 || L.size() != want) fail(label + ": describe lists " + std::to_string(n) + " launches, the call made " + std::to_string(L.size()));
    for (int i = 0; i < n; ++i) {
        const int64_t* r = recs + 4 * i;
        if (!is_kernel(L[i], r[0])) fail(label + ": launch " + std::to_string(i) + " is " + L[i].kernel + ", the plan says kernel " + std::to_string(r[0]));
        if (variant == 3) {
            if (L[i].ptrs[0] != (uintptr_t)a.A) fail(label + ": the slices do not start at A");
            continue;
        }
        const uintptr_t wantA = (uintptr_t)a.A + (uintptr_t)(r[1] * a.lda * 2), wantC = (uintptr_t)a.C + (uintptr_t)(r[1] * a.ldc * 2);
        if (L[i].ptrs.size() < 3 || L[i].ptrs[0] != wantA || L[i].ptrs[2] != wantC)
            fail(label + ": launch " + std::to_string(i) + " does not start at row " + std::to_string(r[1]) + " of A and C: " + rec::describe(L[i]));
    }
    if (variant == 3 && L[n].kernel.find("gemm_splitk_epilogue_kernel<") == std::string::npos) fail(label + ": no reduce launch behind the slices");
    plan_launches += (long)L.size();
    delete[] recs;
}

void plan_case(int force, int64_t M, int64_t N, int64_t K, int64_t rpb) {
    drn_gemm_force_tile(force);
    char head[160];
    snprintf(head, sizeof head, "plan force %d M %lld N %lld K %lld rpb %lld", force, (long long)M, (long long)N, (long long)K, (long long)rpb);
    Gm p;
    p.M = M, p.N = N, p.K = K, p.rpb = rpb;
    for (int epi = 0; epi <= 2; ++epi) {
        p.epi = epi;
        p.rpb = (epi == DRN_EPI_GATE_RES && rpb <= 0) ? M : rpb;
        const std::string h = std::string(head) + " epi " + std::to_string(epi);
        plan_equals_launches(h + " plain", p, 0);
        if (K % 512 == 0) plan_equals_launches(h + " blocked A", p, 1);
        if (N % 512 == 0) plan_equals_launches(h + " blocked C", p, 2);
        if (epi == DRN_EPI_GATE_RES) {                      // ragged clips: the last clip shorter
            Gm r = p;
            r.rpb = M / 2 + 3;
            plan_equals_launches(h + " ragged", r, 0);
            if (N % 512 == 0) plan_equals_launches(h + " ragged blocked C", r, 2);
        }
        Gm s = p;
        const int64_t clip = (rpb > 0 && rpb < M && M % rpb == 0) ? rpb : M;
        for (int splits : {drn_gemm_splitk_choice(clip, N, K), 2, 4, 16})
            if (splits > 1 && M * N * splits < (1ll << 33)) {
                s.splits = splits;
                plan_equals_launches(h + " splits " + std::to_string(splits), s, 3);
            }
    }
    drn_gemm_force_tile(-1);
}

}  // namespace

void gemm_plan_cases(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) fail(std::string("cannot read ") + path);
    long long force, M, N, K, rpb;
    long lines = 0;
    while (fscanf(f, "%lld %lld %lld %lld %lld", &force, &M, &N, &K, &rpb) == 5) {
        plan_case((int)force, M, N, K, rpb);
        ++lines;
    }
    fclose(f);
    if (drn_gemm_force_res_prefetch(-1) != 1 || drn_gemm_tall_force_shape(-1) != -1) fail("a GEMM force knob does not read its default");
    drn_gemm_tall_force_shape(-1);
    printf("plans lines %ld products %ld launches %ld refusals %ld\n", lines, plan_cases, plan_launches, plan_refusals);
}

void family_gemm() {
    const std::vector<Change<Gm>> g_ref = {
        CH(Gm, "null A", p.A = 0), CH(Gm, "null W", p.W = 0), CH(Gm, "null C", p.C = 0), CH(Gm, "M < 0", p.M = -1), CH(Gm, "N == 0", p.N = 0),
        CH(Gm, "K == 0", p.K = 0), CH(Gm, "K % 64", p.K = 4128), CH(Gm, "N % 128", p.N = 4160), CH(Gm, "lda % 8", p.lda = 4100), CH(Gm, "ldw % 8", p.ldw = 4100),
        CH(Gm, "ldc % 8", p.ldc = 4100), CH(Gm, "ldw < K", p.ldw = 4088), CH(Gm, "A off 16 bytes", p.A_mis = 8), CH(Gm, "W off 16 bytes", p.W_mis = 8),
        CH(Gm, "C off 16 bytes", p.C_mis = 8), CH(Gm, "gated residual without gate", p.gate = 0), CH(Gm, "gated residual without residual", p.res = 0),
        CH(Gm, "residual off 8 bytes", p.R_mis = 4), CH(Gm, "ldr % 8", p.ldr = 4100), CH(Gm, "ldr < N", p.ldr = 4088),
        CH(Gm, "gated residual with rows_per_batch == 0", p.rpb = 0), CH(Gm, "epilogue 3", p.epi = 3), CH(Gm, "epilogue -1", p.epi = -1)};
    {
        auto r = g_ref;
        r.push_back(CH(Gm, "lda < K", p.lda = 4088));
        r.push_back(CH(Gm, "ldc < N", p.ldc = 4088));
        entry<Gm>("drn_gemm_bf16", gemm, r,
                  {CH(Gm, "M == 0", p.M = 0), CH(Gm, "no epilogue, no gate", (p.epi = 0, p.gate = 0, p.res = 0)), CH(Gm, "GELU", p.epi = 1),
                   CH(Gm, "18432 rows: 384-row tile", (p.M = 18432, p.rpb = 18432, p.K = 16384)), CH(Gm, "18432 x 16384: tail split", (p.M = 18432, p.rpb = 18432, p.N = 16384)),
                   CH(Gm, "two clips", (p.M = 4608)), CH(Gm, "ragged clips", p.rpb = 1000), CH(Gm, "N 384: 128 x 128 tiles", p.N = 384), CH(Gm, "one row", (p.M = 1, p.rpb = 1)),
                   CH(Gm, "few tokens", (p.M = 256, p.rpb = 256, p.N = 12288)), CH(Gm, "strided A, C and R", (p.lda = 8192, p.ldc = 12288, p.ldr = 8192))},
                  // D: rows either side of 2^31 / tiles either side of the grid limit, operands up to ~250 GB
                  {CH(Gm, "M 2^24: A, C, R of 2^31 elements", (p.M = 1 << 24, p.N = 128, p.K = 128, p.rpb = 1 << 24, p.ldr = 128)),
                   CH(Gm, "M 2^25 + 1", (p.M = (1 << 25) + 1, p.N = 128, p.K = 128, p.rpb = 1 << 20, p.ldr = 128)),
                   CH(Gm, "M 2^29, N 256 (256 GiB of C)", (p.M = G / 2, p.N = 256, p.K = 64, p.rpb = G / 2, p.ldr = 256)),
                   CH(Gm, "M 2^31, N 128", (p.M = 2 * G, p.N = 128, p.K = 64, p.epi = 0)), CH(Gm, "M 2^31 + 128, N 256", (p.M = 2 * G + 128, p.N = 256, p.K = 64, p.epi = 0)),
                   CH(Gm, "2^31 tiles of 128 x 128", (p.M = 1 << 27, p.N = 256 * 1024, p.K = 64, p.epi = 0, p.N = 128 * 2048 + 128))});
        r = g_ref;
        r.push_back(CH(Gm, "a_block_cols not a power of two", p.a_cols = 768));
        r.push_back(CH(Gm, "a_block_cols < 64", p.a_cols = 32));
        r.push_back(CH(Gm, "a_block_cols does not divide K", (p.a_cols = 8192)));
        r.push_back(CH(Gm, "a_block_stride % 8", p.a_stride = 2304 * 512 + 4));
        r.push_back(CH(Gm, "lda < a_block_cols", p.lda = 256));
        r.push_back(CH(Gm, "c_block_cols < 256", p.c_cols = 128));
        r.push_back(CH(Gm, "c_block_cols not a power of two", p.c_cols = 768));
        r.push_back(CH(Gm, "c_block_stride % 8", p.c_stride = 2304 * 512 + 4));
        r.push_back(CH(Gm, "ldc < c_block_cols", p.ldc = 256));
        r.push_back(CH(Gm, "the 128 x 128 kernel's shape", p.N = 384 + 128));
        r.push_back(CH(Gm, "plain A with lda < K", (p.a_cols = 0, p.lda = 4088)));
        r.push_back(CH(Gm, "plain C with ldc < N", (p.c_cols = 0, p.ldc = 4088)));
        entry<Gm>("drn_gemm_bf16_blocked", gemm_blocked, r,
                  {CH(Gm, "plain A", p.a_cols = 0), CH(Gm, "plain C", p.c_cols = 0), CH(Gm, "both plain", (p.a_cols = 0, p.c_cols = 0)), CH(Gm, "no epilogue", p.epi = 0),
                   CH(Gm, "ragged clips", p.rpb = 1000), CH(Gm, "two clips", p.M = 4608), CH(Gm, "K|V projection: N 8192 in planes of 1024", (p.N = 8192, p.c_cols = 1024, p.epi = 0))});
    }
    {
        std::vector<Change<GmS>> r = {
            CH(GmS, "null A", p.A = 0), CH(GmS, "null W", p.W = 0), CH(GmS, "null C", p.C = 0), CH(GmS, "null workspace", p.ws = 0), CH(GmS, "M == 0", p.M = 0),
            CH(GmS, "N == 0", p.N = 0), CH(GmS, "K == 0", p.K = 0), CH(GmS, "splits 65", p.splits = 65), CH(GmS, "K % 64", p.K = 4128), CH(GmS, "N % 128", p.N = 4160),
            CH(GmS, "K steps % splits", p.splits = 3), CH(GmS, "lda % 8", p.lda = 4100), CH(GmS, "ldw % 8", p.ldw = 4100), CH(GmS, "ldc % 8", p.ldc = 4100),
            CH(GmS, "lda < K", p.lda = 4088), CH(GmS, "ldw < K", p.ldw = 4088), CH(GmS, "ldc < N", p.ldc = 4088), CH(GmS, "A off 16 bytes", p.A_mis = 8),
            CH(GmS, "W off 16 bytes", p.W_mis = 8), CH(GmS, "C off 16 bytes", p.C_mis = 8), CH(GmS, "workspace off 16 bytes", p.ws_mis = 8),
            CH(GmS, "no gate", p.gate = 0), CH(GmS, "no residual", p.res = 0), CH(GmS, "ldr % 8", p.ldr = 4100), CH(GmS, "ldr < N", p.ldr = 4088),
            CH(GmS, "rows_per_batch == 0", p.rpb = 0), CH(GmS, "residual off 8 bytes", p.R_mis = 4), CH(GmS, "epilogue 3", p.epi = 3),
            CH(GmS, "65536 tiles of slices", (p.M = 128 * 512, p.N = 128 * 128, p.K = 128, p.splits = 2, p.rpb = 128 * 512))};
        entry<GmS>("drn_gemm_bf16_splitk", gemm_splitk, r,
                   {CH(GmS, "splits 1: the plain entry", p.splits = 1), CH(GmS, "MLP-down: 16 slices", (p.N = 4096, p.K = 16384, p.splits = 16)),
                    CH(GmS, "QKV: 256-row slices", (p.N = 12288, p.splits = 4)), CH(GmS, "128 x 128 slices", (p.M = 200, p.rpb = 200, p.splits = 2)),
                    CH(GmS, "GELU", p.epi = 1), CH(GmS, "three clips", (p.M = 768)), CH(GmS, "65535 tiles of slices", (p.M = 128 * 257, p.N = 128 * 255, p.K = 128, p.splits = 2, p.rpb = 128 * 257))});
        r.erase(std::remove_if(r.begin(), r.end(),
                               [](const Change<GmS>& c) {
                                   for (const char* k : {"null C", "ldc", "C off", "gate", "residual", "ldr", "rows_per_batch", "epilogue"})
                                       if (strstr(c.what, k)) return true;
                                   return false;
                               }),
                r.end());
        r.push_back(CH(GmS, "splits 1", p.splits = 1));
        entry<GmS>("drn_gemm_bf16_splitk_partials", gemm_partials, r, {CH(GmS, "MLP-down: 16 slices", (p.N = 4096, p.K = 16384, p.splits = 16)), CH(GmS, "splits 64", (p.splits = 64))});
    }
    entry<GmF>("drn_gemm_bf16_f32out", gemm_f32,
               {CH(GmF, "null A", p.A = 0), CH(GmF, "null W", p.W = 0), CH(GmF, "null C", p.C = 0), CH(GmF, "M == 0", p.M = 0), CH(GmF, "M % 256", p.M = 9216 + 128),
                CH(GmF, "N % 256", p.N = 9216 + 128), CH(GmF, "K % 64", p.K = 544), CH(GmF, "K == 0", p.K = 0), CH(GmF, "lda % 8", p.lda = 516), CH(GmF, "lda < K", p.lda = 504),
                CH(GmF, "ldw < K", p.ldw = 504), CH(GmF, "A off 16 bytes", p.A_mis = 8), CH(GmF, "W off 16 bytes", off("W", 8)), CH(GmF, "C off 16 bytes", p.C_mis = 8),
                CH(GmF, "65536 tiles", (p.M = 65536, p.N = 65536))},
               {CH(GmF, "one tile", (p.M = 256, p.N = 256)), CH(GmF, "65535 tiles (16 GiB of C)", (p.M = 256 * 255, p.N = 256 * 257))});

    // ---- MXFP8
    const std::vector<Change<Mx>> mx_ref = {
        CH(Mx, "null A", p.A = 0), CH(Mx, "null SA", p.SA = 0), CH(Mx, "null W", p.W = 0), CH(Mx, "null SW", p.SW = 0), CH(Mx, "null C", p.C = 0), CH(Mx, "M == 0", p.M = 0),
        CH(Mx, "N == 0", p.N = 0), CH(Mx, "N % 256", p.N = 4224), CH(Mx, "K == 0", p.K = 0), CH(Mx, "K % 128", p.K = 4160), CH(Mx, "ldc % 4", p.ldc = 4098),
        CH(Mx, "C off 8 bytes", p.C_mis = 4), CH(Mx, "A off 16 bytes", p.A_mis = 8), CH(Mx, "W off 16 bytes", p.W_mis = 8), CH(Mx, "SA off 4 bytes", p.SA_mis = 2),
        CH(Mx, "SW off 4 bytes", p.SW_mis = 2), CH(Mx, "no gate", p.gate = 0), CH(Mx, "no residual", p.res = 0), CH(Mx, "ldr < N", p.ldr = 4092), CH(Mx, "ldr % 4", p.ldr = 4162),
        CH(Mx, "residual off 8 bytes", p.R_mis = 4), CH(Mx, "gate off 8 bytes", p.G_mis = 4), CH(Mx, "epilogue 3", p.epi = 3),
        CH(Mx, "2^31 tiles", (p.M = 256ll << 16, p.N = 256ll << 15, p.K = 128, p.epi = 0))};
    {
        auto r = mx_ref;
        r.push_back(CH(Mx, "ldc < N", p.ldc = 4092));
        entry<Mx>("drn_gemm_mxfp8", mx, r,
                  {CH(Mx, "one row", (p.M = 1, p.rpb = 1)), CH(Mx, "no epilogue", (p.epi = 0, p.gate = 0, p.res = 0)), CH(Mx, "GELU", p.epi = 1), CH(Mx, "rows_per_batch 0: one clip", p.rpb = 0),
                   CH(Mx, "ragged rows", p.M = 2305), CH(Mx, "18432 x 16384", (p.M = 18432, p.N = 16384, p.rpb = 18432)),
                   CH(Mx, "2^31 - 2^16 tiles", (p.M = (256ll << 16) - 256, p.N = 256ll << 15, p.K = 128, p.epi = 0))});
        r = mx_ref;
        r.push_back(CH(Mx, "a_block_cols % 128", p.a_cols = 64));
        r.push_back(CH(Mx, "a_block_cols does not divide K", p.a_cols = 1536));
        r.push_back(CH(Mx, "a_block_stride % 128", p.a_stride = 2304 * 512 + 64));
        r.push_back(CH(Mx, "a_block_stride < M a_block_cols", p.a_stride = 2303 * 512));
        r.push_back(CH(Mx, "c_block_cols not a power of two", p.c_cols = 768));
        r.push_back(CH(Mx, "c_block_cols < 256", p.c_cols = 128));
        r.push_back(CH(Mx, "c_block_cols does not divide N", (p.c_cols = 8192)));
        r.push_back(CH(Mx, "ldc < c_block_cols", p.ldc = 256));
        r.push_back(CH(Mx, "c_block_stride % 4", p.c_stride = 2304 * 512 + 2));
        r.push_back(CH(Mx, "c planes overlap", p.c_stride = 2303 * 512 + 508));
        r.push_back(CH(Mx, "plain C with ldc < N", (p.c_cols = 0, p.ldc = 4092)));
        entry<Mx>("drn_gemm_mxfp8_blocked", mx_blocked, r,
                  {CH(Mx, "plain A", p.a_cols = 0), CH(Mx, "plain C", p.c_cols = 0), CH(Mx, "both plain", (p.a_cols = 0, p.c_cols = 0)), CH(Mx, "ragged rows", p.M = 2305),
                   CH(Mx, "planes that just do not overlap", p.c_stride = 2303 * 512 + 512), CH(Mx, "no epilogue", p.epi = 0)});
    }
    {
        std::vector<Change<MxS>> r = {
            CH(MxS, "null A", p.A = 0), CH(MxS, "null SA", p.SA = 0), CH(MxS, "null W", p.W = 0), CH(MxS, "null SW", p.SW = 0), CH(MxS, "null workspace", p.ws = 0),
            CH(MxS, "M % 256", p.M = 384), CH(MxS, "M == 0", p.M = 0), CH(MxS, "more than 1024 rows per clip", (p.M = 1280, p.rpb = 1280)), CH(MxS, "N % 256", p.N = 4224),
            CH(MxS, "K % 128", p.K = 4160), CH(MxS, "K steps % splits", p.splits = 3), CH(MxS, "splits 0", p.splits = 0), CH(MxS, "splits 128", (p.splits = 128, p.K = 16384)),
            CH(MxS, "A off 16 bytes", p.A_mis = 8), CH(MxS, "W off 16 bytes", p.W_mis = 8), CH(MxS, "SA off 4 bytes", p.SA_mis = 2), CH(MxS, "SW off 4 bytes", p.SW_mis = 2),
            CH(MxS, "workspace off 16 bytes", p.ws_mis = 8), CH(MxS, "33 K >= 2^32", (p.K = 1ll << 27, p.N = 256, p.splits = 2))};
        auto rp = r;
        rp.push_back(CH(MxS, "splits 1", p.splits = 1));
        r.push_back(CH(MxS, "null C", p.C = 0));
        r.push_back(CH(MxS, "ldc < N", p.ldc = 4092));
        r.push_back(CH(MxS, "ldc % 4", p.ldc = 4098));
        r.push_back(CH(MxS, "C off 8 bytes", p.C_mis = 4));
        r.push_back(CH(MxS, "epilogue 3", p.epi = 3));
        r.push_back(CH(MxS, "no gate", p.gate = 0));
        r.push_back(CH(MxS, "no residual", p.res = 0));
        r.push_back(CH(MxS, "ldr < N", p.ldr = 4092));
        r.push_back(CH(MxS, "residual off 8 bytes", p.R_mis = 4));
        r.push_back(CH(MxS, "gate off 8 bytes", p.G_mis = 4));
        entry<MxS>("drn_gemm_mxfp8_splitk", mx_splitk, r,
                   {CH(MxS, "splits 1: fused", (p.splits = 1, p.ws = 0)), CH(MxS, "splits 64", (p.splits = 64, p.K = 16384)), CH(MxS, "four clips of 1024", (p.M = 4096, p.rpb = 1024)),
                    CH(MxS, "GELU", p.epi = 1), CH(MxS, "no epilogue", (p.epi = 0, p.gate = 0, p.res = 0)),
                    CH(MxS, "many clips: 2^22 rows", (p.M = 1 << 22, p.rpb = 1024, p.N = 256, p.K = 256, p.splits = 2))});
        entry<MxS>("drn_gemm_mxfp8_splitk_partials", mx_partials, rp, {CH(MxS, "splits 2", p.splits = 2), CH(MxS, "four clips of 1024", (p.M = 4096, p.rpb = 1024))});
    }
    entry<MxG>("drn_gemm_mxfp8_gelu_mx", mx_gelu,
               {CH(MxG, "null A", p.A = 0), CH(MxG, "null SA", p.SA = 0), CH(MxG, "null W", p.W = 0), CH(MxG, "null SW", p.SW = 0), CH(MxG, "null CQ", p.C = 0), CH(MxG, "null CS", p.CS = 0),
                CH(MxG, "M == 0", p.M = 0), CH(MxG, "N % 256", p.N = 16512), CH(MxG, "K % 128", p.K = 4160), CH(MxG, "A off 16 bytes", p.A_mis = 8), CH(MxG, "W off 16 bytes", p.W_mis = 8),
                CH(MxG, "SA off 4 bytes", p.SA_mis = 2), CH(MxG, "SW off 4 bytes", p.SW_mis = 2), CH(MxG, "CQ off 4 bytes", p.C_mis = 2),
                CH(MxG, "a shape whose choice slices K", (p.M = 256, p.rpb = 256, p.N = 4096)), CH(MxG, "2^31 tiles", (p.M = 256ll << 16, p.N = 256ll << 15, p.K = 128, p.rpb = 0))},
               {CH(MxG, "few tokens: the fused few-token kernel", (p.M = 256, p.rpb = 256)), CH(MxG, "two clips of 256", (p.M = 512, p.rpb = 256)), CH(MxG, "ragged rows", (p.M = 2305, p.rpb = 0)),
                CH(MxG, "18432 rows", (p.M = 18432, p.rpb = 18432))});
}

}  // namespace hw
