// host walk, section E: the host-only entries - sizers, choices, plans - swept over small, model and huge arguments.  They must return
// without a sanitizer report, and a sizer returns 0 exactly where its entry refuses.  "Huge" stops where the bytes an argument list
// stands for pass 2^56: beyond that the products leave int64, and no caller can hold such a tensor.
#include "host_walk.h"

namespace hw {
namespace {

const int64_t kVals[] = {-1, 0, 1, 2, 127, 128, 255, 256, 257, 1024, 2304, 4096, 18432, 65535, 65536, (1ll << 31) - 1, 1ll << 31, (1ll << 32) + 1};
const int kInts[] = {-1, 0, 1, 2, 3, 16, 17, 64, 255, 256, 4096, 65535, 65536, 0x7fffffff};
const double kLimit = 72057594037927936.0;   // 2^56

bool fits(std::initializer_list<int64_t> v, double scale = 1.0) {
    double p = scale;
    for (int64_t x : v) p *= x > 1 ? (double)x : 1.0;
    return p < kLimit;
}

int refuses(const std::function<int()>& fn) {
    rec::reset();
    const int rc = fn();
    if (rc == DRN_EINVAL && (!rec::launches().empty() || !rec::attrs().empty())) fail("section E: a refusal after a launch");
    if (rc != DRN_EINVAL && rc != DRN_OK) fail("section E: an entry returns " + std::to_string(rc));
    if (rc == DRN_OK) {
        const std::string bad = rec::check_call();
        if (!bad.empty()) fail("section E: " + bad);
    }
    return rc == DRN_EINVAL;
}

}  // namespace

void family_host_only() {
    long calls = 0, pairs = 0;
    if (drn_abi_version() != DRN_ABI_VERSION || !drn_error_string(0) || !drn_error_string(-1) || !drn_error_string(98) || !drn_error_string(-77)) fail("abi / error string");
    if (drn_dit_forward_args_bytes() != (int64_t)sizeof(drn_dit_forward_args) || drn_dit_sub_bytes() != (int64_t)sizeof(drn_dit_sub)) fail("struct sizes");
    int kt = 0, pexp = 0;
    float thr = 0.f;
    if (drn_attention_mxfp8_params(&kt, &thr, &pexp) != DRN_OK || drn_attention_mxfp8_params(nullptr, &thr, &pexp) != DRN_EINVAL) fail("drn_attention_mxfp8_params");
    calls += 8;

    // ---- GEMM choices and plans
    for (int64_t M : kVals)
        for (int64_t N : kVals)
            for (int64_t K : kVals) {
                if (!fits({M, N, K})) continue;
                drn_gemm_tile_choice(M, N);
                drn_gemm_splitk_choice(M, N, K);
                drn_gemm_mxfp8_splitk_choice(M, N, K);
                int64_t main_rows = -7;
                for (int64_t rpb : {(int64_t)0, (int64_t)256, M / 2, M, M + 1}) {
                    const int rc = drn_gemm_plan_choice(M, N, K, rpb, &main_rows);
                    if (rc == DRN_EINVAL ? main_rows != 0 : (main_rows < 1 || main_rows > M)) fail("drn_gemm_plan_choice: main_rows outside the clip");
                    drn_gemm_plan_choice(M, N, K, rpb, nullptr);
                    int64_t* recs = new int64_t[4 * 3];          // cap 3: describe may not write a fourth record
                    for (int splits : {1, 2, 64, 65})
                        for (int epi : {0, 2, 3}) {
                            const int n = drn_gemm_plan_describe(M, N, K, K, K, N, N, epi, rpb, 0, 0, splits, recs, 3);
                            if (n < -1) fail("drn_gemm_plan_describe returns below -1");
                            drn_gemm_plan_describe(M, N, K, K, K, N, N, epi, rpb, 0, 0, splits, nullptr, 0);
                            calls += 2;
                        }
                    delete[] recs;
                    calls += 2;
                }
                for (int splits : kInts)
                    if (fits({M, N, splits}, 4.0)) {
                        const int64_t b = drn_gemm_splitk_workspace_bytes(M, N, splits);
                        if (splits <= 1 ? b != 0 : (M > 0 && N > 0 && b != (int64_t)splits * M * N * 4)) fail("drn_gemm_splitk_workspace_bytes");
                        ++calls;
                    }
                calls += 3;
            }

    // ---- attention: plan, choice, workspace
    for (int heads : kInts)
        for (int64_t Sq : kVals)
            for (int64_t Sk : kVals) {
                if (heads > 65536 || !fits({heads, Sq, Sk})) continue;
                int64_t* plan = new int64_t[6];
                for (int i = 0; i < 6; ++i) plan[i] = -5;
                const int n = drn_attention_plan(heads, Sq, Sk, plan);
                const bool valid = heads > 0 && Sq > 0 && Sk > 0;
                if (valid ? (n < 1 || n > 2 || plan[0] != 0 || plan[3 * n - 2] != Sq || (n == 2 && plan[1] != plan[3])) : n != 0) fail("drn_attention_plan does not tile [0, Sq)");
                for (int i = 0; i < n; ++i)
                    if (plan[3 * i + 2] < 1 || plan[3 * i + 2] > 64) fail("drn_attention_plan: a split count outside 1..64");
                delete[] plan;
                if (drn_attention_plan(heads, Sq, Sk, nullptr) != 0) fail("drn_attention_plan with a null plan");
                drn_attention_mxfp8_choice(heads, Sq);
                for (int batch : {1, 3, 65535})
                    for (int ns : {1, 2, 64})
                        if (fits({batch, heads, Sq, ns}, 520.0)) drn_attention_splitkv_workspace_bytes(batch, heads, Sq, ns), ++calls;
                calls += 3;
            }

    // ---- the forward's sizers
    for (int64_t B : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)65535, (int64_t)65536})
        for (int64_t S : kVals)
            for (int64_t D : {(int64_t)-128, (int64_t)0, (int64_t)100, (int64_t)128, (int64_t)256, (int64_t)2048, (int64_t)4096, (int64_t)8192, (int64_t)1 << 20}) {
                if (!fits({B, S, D}, 64.0)) continue;
                const int64_t hid = 4 * D;
                drn_dit_forward_gemm_workspace_bytes(B, S, D, hid, 128, 192);
                drn_dit_forward_mx_gemm_workspace_bytes(B, S, D, hid);
                drn_dit_forward_mx_act_bytes(B, S, D, hid);
                drn_dit_forward_mx_u_bytes(B, S, hid);
                if (D > 0 && D % 128 == 0 && D / 128 <= 65536 && B <= 65535) drn_dit_forward_attn_workspace_bytes(B, (int)(D / 128), S);
                int64_t* lay = new int64_t[8];
                const int rc = drn_dit_forward_mx_attn_layout(B, S, D, lay);
                const int64_t bytes = drn_dit_forward_mx_attn_bytes(B, S, D);
                if ((rc == DRN_EINVAL) != (bytes == 0) || (rc == DRN_OK && (lay[6] != bytes || lay[0] != 0 || lay[7] < S || lay[7] % 128 != 0)))
                    fail("drn_dit_forward_mx_attn_bytes is not 0 exactly where the layout is refused");
                for (int i = 1; rc == DRN_OK && i < 7; ++i)
                    if (lay[i] % 256 != 0 || lay[i] <= lay[i - 1]) fail("drn_dit_forward_mx_attn_layout: offsets not ascending on 256 bytes");
                delete[] lay;
                if (drn_dit_forward_mx_attn_layout(B, S, D, nullptr) != DRN_EINVAL) fail("drn_dit_forward_mx_attn_layout with a null out");
                calls += 8, ++pairs;
            }

    // ---- sizers that belong to a launching entry: 0 exactly where the entry refuses (operands otherwise valid)
    for (int B : kInts)
        for (int64_t n : kVals) {
            if (!fits({B, n}, 2.0)) continue;
            const int64_t ws = drn_step_cache_workspace_bytes(B, n);
            const int r = refuses([&] {
                return drn_step_cache_probe(A("x", (int64_t)B * n * 2), A("ref", (int64_t)B * n * 2), A("stats", (int64_t)B * 16), A("workspace", ws ? ws : 8), ws, B, n, STREAM);
            });
            if ((ws == 0) != (r == 1)) fail("drn_step_cache_workspace_bytes(" + std::to_string(B) + ", " + std::to_string(n) + ") = " + std::to_string(ws) + " but the probe " + (r ? "refuses" : "runs"));
            ++calls, ++pairs;
        }
    for (int B : kInts)
        for (int H : {-1, 0, 1, 45, 704, 65536})
            for (int W : {0, 1, 37, 1280, 65536})
                for (int O : {-1, 0, 1, 3, 4096}) {
                    if (!fits({B, H, W, O}, 6.0)) continue;
                    const int64_t ws = drn_window_align_workspace_bytes(B, H, W, O);
                    const int64_t hw = (int64_t)H * W;
                    const int r = refuses([&] {
                        return drn_window_align_affine(A("video", (int64_t)B * 3 * O * hw * 2), A("prev_tail", (int64_t)B * 3 * O * hw * 2), A("affine", (int64_t)B * 8), nullptr,
                                                       A("workspace", ws ? ws : 8), ws, B, O, H, W, O, 0, STREAM);
                    });
                    // the sizer is "0 for a non-positive size"; the entry refuses more (B > 65535, too many chunks): one direction
                    if (ws == 0 && !r) fail("drn_window_align_workspace_bytes is 0 for a size the entry takes");
                    if (ws != 0 && r && B <= 65535 && 3 * ((int64_t)O * hw + 8191) / 8192 < (1ll << 31)) fail("drn_window_align_affine refuses a size its sizer and header allow");
                    ++calls, ++pairs;
                }
    for (int N : {-1, 0, 1, 2, 3, 16, 17})
        for (int B : kInts)
            for (int64_t cb : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)16, (int64_t)8192, (int64_t)8193, (int64_t)1 << 31, (int64_t)1 << 36, ((int64_t)1 << 36) + 1}) {
                if (B > 65536 && cb > (1ll << 31)) continue;
                const int64_t ws = drn_ensemble_align_workspace_bytes(N, B, cb);
                const int n = N > 0 && N <= 16 ? N : 1;
                const void** members = new const void*[n];
                for (int k = 0; k < n; ++k) members[k] = (const void*)(uintptr_t)(0x100000 * (k + 1));     // fake and never read: only the table is
                const int r = refuses([&] {
                    for (int k = 0; k < n; ++k) members[k] = A("member", B > 0 && cb > 0 && fits({B, cb}) ? (int64_t)B * cb : 1);
                    return drn_ensemble_align_affine(members, N, B, cb, A("affine", 16 * 65536 * 8), nullptr, A("workspace", ws ? ws : 8), ws, STREAM);
                });
                delete[] members;
                if ((ws == 0) != (r == 1)) fail("drn_ensemble_align_workspace_bytes is not 0 exactly where the entry refuses");
                ++calls, ++pairs;
            }
    for (int frames : kInts) drn_groupnorm_workspace_bytes(frames), ++calls;
    drn_mx_quant_calls(0), drn_conv_last_tile(), drn_attention_mx_available();
    // the timer: the one object the library allocates
    for (int cap : {-1, 0, 1, 8}) {
        void* t = drn_timer_create(cap, cap);
        int kind = 0;
        float ms = 0.f;
        double fl = 0., by = 0.;
        if ((t == nullptr) != (cap <= 0) || drn_timer_count(t) != 0 || drn_timer_seen(t, 0) != 0 || drn_timer_seen(t, 2) != 0 || drn_timer_read(t, 0, &kind, &ms, &fl, &by) != DRN_EINVAL)
            fail("drn_timer_*");
        drn_timer_destroy(t);
        calls += 6;
    }
    tally.host_only = calls;
    printf("host-only calls %ld sizer / entry pairs %ld\n", calls, pairs);
}

}  // namespace hw
