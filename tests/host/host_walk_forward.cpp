// host walk, section C: the forward sequencer.  drn_dit_forward_args is built the way dit_engine.py builds it - the sub-block table a
// real heap block of exactly n_sub entries, every device operand an arena of its exact size, the workspaces sized by the sizers -
// and drn_dit_forward / drn_dit_forward_range are walked: exact workspaces, one byte short, every cut, reruns, injected failures.
// Also section B for attention: the plan's ranges are what a self-attention sub-block launches.
#include <string.h>

#include "host_walk.h"

namespace hw {
namespace {

struct Net {
    int64_t D, hidden;
    int L, heads;
    int64_t S, B;
    int precision = 0, mx_fused = 0, attn_precision = 0;
    int64_t kpad = 192, n_final = 128;
    const char* kinds = "fcm";          // the sub-blocks of one block: f FA, c CA, m MLP
    // single changes for the refusal cases
    int64_t short_gemm = 0, short_attn = 0, short_act = 0, short_u = 0, short_mxa = 0;
    bool with_timer = false;
};

// the argument block and what owns its host memory
struct Built {
    drn_dit_forward_args a;
    drn_dit_sub* subs = nullptr;
    int n_sub = 0;
    void* timer = nullptr;
    int64_t need_gemm = 0, need_attn = 0;
    ~Built() {
        delete[] subs;
        if (timer) drn_timer_destroy(timer);
    }
};

void build(const Net& n, Built* b) {
    rec::reset();
    delete[] b->subs;                                    // (a Built may be built again: same arenas in the same order, same addresses)
    if (b->timer) drn_timer_destroy(b->timer);
    b->timer = nullptr;
    drn_dit_forward_args& a = b->a;
    memset(&a, 0, sizeof a);
    const int64_t D = n.D, hid = n.hidden, S = n.S, B = n.B, M = B * S;
    const bool mx = n.precision == 1;
    const int per = (int)strlen(n.kinds);
    b->n_sub = n.L * per;
    b->subs = b->n_sub ? new drn_dit_sub[b->n_sub] : nullptr;        // exactly n_sub entries: a read one past it is ASan's
    // weights never move after load; every block's are the same size, so one arena per kind stands for all blocks
    void* w_qkv = A("w_qkv", 3 * D * D * (mx ? 1 : 2));
    void* w_o = A("w_o", D * D * (mx ? 1 : 2));
    void* w_1 = A("w_mlp1", hid * D * (mx ? 1 : 2));
    void* w_2 = A("w_mlp2", D * hid * (mx ? 1 : 2));
    void* s_qkv = mx ? A("s_qkv", 3 * D * D / 32) : nullptr;
    void* s_o = mx ? A("s_o", D * D / 32) : nullptr;
    void* s_1 = mx ? A("s_mlp1", hid * D / 32) : nullptr;
    void* s_2 = mx ? A("s_mlp2", D * hid / 32) : nullptr;
    void* qn = A("qn", 256);
    void* kn = A("kn", 256);
    int n_ca = 0;
    for (int i = 0; i < b->n_sub; ++i) {
        drn_dit_sub& e = b->subs[i];
        memset(&e, 0, sizeof e);
        e.site = i, e.ca_index = -1;
        const char kind = n.kinds[i % per];
        if (kind == 'f') e.kind = DRN_SUB_FA, e.w_a = w_qkv, e.w_b = w_o, e.s_a = s_qkv, e.s_b = s_o, e.qn = qn, e.kn = kn;
        else if (kind == 'c') e.kind = DRN_SUB_CA, e.ca_index = n_ca++;
        else e.kind = DRN_SUB_MLP, e.w_a = w_1, e.w_b = w_2, e.s_a = s_1, e.s_b = s_2;
    }
    a.struct_bytes = (int64_t)sizeof a;
    a.S = S, a.B = B, a.D = D, a.hidden = hid, a.heads = n.heads, a.n_sub = b->n_sub, a.subs = b->subs;
    // AdaLN vectors of a batch: shift | scale rows [sites][2][B][D], gates [sites][B][D] (dit_engine.HipDiT._forward_args)
    char* modB = (char*)A("modB", (int64_t)(b->n_sub + 1) * 2 * B * D * 2);
    a.shift = modB, a.scale = modB + B * D * 2, a.gate = A("gateB", (int64_t)(b->n_sub ? b->n_sub : 1) * B * D * 2);
    a.shift_site_stride = a.scale_site_stride = 2 * B * D, a.gate_site_stride = B * D;
    a.final_shift = modB + (int64_t)b->n_sub * 2 * B * D * 2, a.final_scale = (const char*)a.final_shift + B * D * 2;
    a.addvec = n_ca ? A("addvec", (int64_t)n_ca * B * D * 2) : nullptr, a.addvec_stride = B * D;
    a.cos = A("cos", S * 256), a.sin = A("sin", S * 256);
    a.P = A("P", M * n.kpad * 2), a.kpad = n.kpad, a.w_patch = A("w_patch", D * n.kpad * 2);
    a.w_final = A("w_final", n.n_final * D * 2), a.n_final = n.n_final;
    a.X = A("X", M * D * 2), a.H = A("H", M * D * 2), a.QKV = A("QKV", M * 3 * D * 2), a.O = A("O", M * D * 2);
    a.U = A("U", M * hid * 2), a.Y = A("Y", M * n.n_final * 2);
    a.eps = 1e-6f, a.precision = n.precision, a.mx_fused = n.mx_fused, a.attn_precision = n.attn_precision;
    int64_t need = drn_dit_forward_gemm_workspace_bytes(B, S, D, hid, n.n_final, n.kpad);
    if (mx) {
        // drn.h: "precision 1: the larger of its patch-embed / final-layer share and drn_dit_forward_mx_gemm_workspace_bytes" - the
        // share of a bf16 linear [M, N, K] is the slices of its split, chosen from one clip's rows (all public entries)
        auto share = [&](int64_t N, int64_t K) { return drn_gemm_splitk_workspace_bytes(M, N, S <= 1024 ? drn_gemm_splitk_choice(S, N, K) : 1); };
        need = drn_dit_forward_mx_gemm_workspace_bytes(B, S, D, hid);
        for (const int64_t v : {share(D, n.kpad), share(n.n_final, D)}) need = v > need ? v : need;
    }
    b->need_gemm = need;
    a.gemm_ws_bytes = need - n.short_gemm;
    a.gemm_ws = need ? A("gemm_ws", a.gemm_ws_bytes) : nullptr;
    b->need_attn = drn_dit_forward_attn_workspace_bytes(B, n.heads, S);
    a.attn_ws_bytes = b->need_attn - n.short_attn;
    a.attn_ws = b->need_attn ? A("attn_ws", a.attn_ws_bytes) : nullptr;
    if (mx) {
        const int64_t k = D > hid ? D : hid;
        a.act_bytes = drn_dit_forward_mx_act_bytes(B, S, D, hid) - n.short_act;
        char* act = (char*)A("act", a.act_bytes);        // AQ | AS in one buffer, the scales behind M x max(D, hidden) elements
        a.AQ = act, a.AS = act + M * k;
    }
    if (n.mx_fused) {
        a.u_act_bytes = drn_dit_forward_mx_u_bytes(B, S, hid) - n.short_u;
        char* u = (char*)A("uact", a.u_act_bytes);
        a.UQ = u, a.US = u + M * hid;
    }
    if (n.attn_precision) {
        a.mx_attn_bytes = drn_dit_forward_mx_attn_bytes(B, S, D) - n.short_mxa;
        a.mx_attn = A("mx_attn", a.mx_attn_bytes);
    }
    if (n.with_timer) a.timer = b->timer = drn_timer_create(8, 3);
}

std::string net_name(const Net& n) {
    char buf[200];
    snprintf(buf, sizeof buf, "D %lld L %d x %s heads %d S %lld B %lld precision %d fused %d attn %d", (long long)n.D, n.L, n.kinds, n.heads,
             (long long)n.S, (long long)n.B, n.precision, n.mx_fused, n.attn_precision);
    return buf;
}

int forward(const Net& n) {
    Built b;
    build(n, &b);
    return drn_dit_forward(&b.a, STREAM);
}

int forced_attmx = 0, forced_body16 = 1;      // what this walk itself set (the two sections below that force a knob)
void knobs_at_default(const std::string& label) {
    const bool ok = drn_gemm_force_res_prefetch(-1) == 1 && drn_gemm_mxfp8_force_small_m(-1) == 1 && drn_attention_mxfp8_force(2) == forced_attmx &&
                    drn_gemm_tall_force_shape(-1) == -1 && drn_gemm_mxfp8_tall_force_shape(-1) == -1 &&
                    drn_gemm_tile_choice(18432, 4096) == 1 && drn_attention_mx_available() == forced_body16;
    if (!ok) fail(label + ": a force knob does not read its default after the call");
}

bool has(const rec::Launch& l, const char* name) { return l.kernel.find(name) != std::string::npos; }

// parts (EMBED, 0..k) + (k..n, FINAL) against the whole forward.  One legitimate difference, at the cut only: where the whole
// forward defers the split-K sum of the sub-block in front of the cut into the next LayerNorm pass (splitk_gate_res_ln_kernel), the
// part completes X itself - the reduce launch (gemm_splitk_epilogue_kernel) ends part one, a plain ln_modulate kernel starts part two.
void compare_cut(const std::string& label, const std::vector<rec::Launch>& whole, const std::vector<rec::Launch>& one, const std::vector<rec::Launch>& two,
                 long* substitutions) {
    std::vector<rec::Launch> parts = one;
    parts.insert(parts.end(), two.begin(), two.end());
    size_t i = 0, j = 0;
    int subst = 0;
    while (i < whole.size() && j < parts.size()) {
        if (whole[i] == parts[j]) { ++i, ++j; continue; }
        const bool at_cut = j + 1 == one.size() && j + 1 < parts.size();
        if (at_cut && subst == 0 && has(whole[i], "splitk_gate_res_ln_kernel") && has(parts[j], "gemm_splitk_epilogue_kernel")) {
            ++subst;
            // the substituted launches work on the fused pass's operands.  Parameters: splitk_gate_res_ln_kernel(partials, splits, n, x,
            // gate, add_vec, shift, scale, h, D, rpb, eps, hq, hs); gemm_splitk_epilogue_kernel(workspace, splits, C, M, N, ldc, gate,
            // residual, ldr, rpb); ln_modulate_kernel(x, add_vec, shift, scale, h, rows, D, rpb, eps, hq, hs)
            const rec::Launch &f = whole[i], &r = parts[j], &l = parts[j + 1];
            if (f.ptrs.size() != 14 || r.ptrs.size() != 10) fail(label + ": the substituted kernels' parameter lists changed");
            if (r.ptrs[0] != f.ptrs[0] || r.ptrs[2] != f.ptrs[3] || r.ptrs[7] != f.ptrs[3] || r.ptrs[6] != f.ptrs[4] || r.stream != f.stream)
                fail(label + ": the reduce at the cut does not work on the fused pass's workspace, X and gate: " + rec::describe(r));
            if (has(l, "ln_modulate_kernel")) {
                if (l.ptrs.size() != 11 || l.ptrs[0] != f.ptrs[3] || l.ptrs[1] != f.ptrs[5] || l.ptrs[2] != f.ptrs[6] || l.ptrs[3] != f.ptrs[7] ||
                    l.ptrs[4] != f.ptrs[8] || l.ptrs[9] != f.ptrs[12] || l.ptrs[10] != f.ptrs[13] || l.stream != f.stream)
                    fail(label + ": the LayerNorm behind the cut does not work on the fused pass's X, add, shift, scale and outputs: " + rec::describe(l));
                ++i, j += 2;
                continue;
            }
            // two cross-attentions behind the cut: the forward's fused pass only completed X (no add; H is scratch), the stand-alone add
            // follows in both lists and is compared like any other launch
            if (has(l, "bcast_add_kernel") && f.ptrs[5] == 0) { ++i, ++j; continue; }
        }
        fail(label + ": launch " + std::to_string(i) + " of the forward is " + rec::describe(whole[i]) + ", of the parts " + rec::describe(parts[j]) + " (part one has " + std::to_string(one.size()) + " launches; next of the parts: " +
             (j + 1 < parts.size() ? parts[j + 1].kernel : std::string("none")) + ")");
    }
    if (i != whole.size() || j != parts.size()) fail(label + ": the parts make " + std::to_string(parts.size()) + " launches, the forward " + std::to_string(whole.size()));
    *substitutions += subst;
}

long cut_cases = 0, cut_substitutions = 0, forward_launches = 0, nets_with_attn_ws = 0;

void walk_net(const Net& n, bool inject) {
    const std::string name = "forward " + net_name(n);
    // 1. exact workspaces
    std::vector<rec::Launch> whole;
    expect_ok(name + ": workspaces as the sizers say", [&] { return forward(n); });
    whole = rec::launches();
    forward_launches += (long)whole.size();
    // 4. the same call again: the same list; the knobs at their defaults
    {
        Built b;
        build(n, &b);
        if (drn_dit_forward(&b.a, STREAM) != DRN_OK || !(rec::launches() == whole)) fail(name + ": a second call records another launch list");
        knobs_at_default(name);
    }
    // 2. one byte less in any single workspace
    {
        Built probe;
        build(n, &probe);
        Net m = n;
        if (probe.need_gemm) { m = n, m.short_gemm = 1; expect_refusal(name + ": gemm_ws one byte short", [&] { return forward(m); }); }
        nets_with_attn_ws += probe.need_attn > 0;
        if (probe.need_attn) { m = n, m.short_attn = 1; expect_refusal(name + ": attn_ws one byte short", [&] { return forward(m); }); }
        if (n.precision) { m = n, m.short_act = 1; expect_refusal(name + ": AQ | AS one byte short", [&] { return forward(m); }); }
        if (n.mx_fused) { m = n, m.short_u = 1; expect_refusal(name + ": UQ | US one byte short", [&] { return forward(m); }); }
        if (n.attn_precision) { m = n, m.short_mxa = 1; expect_refusal(name + ": mx_attn one byte short", [&] { return forward(m); }); }
    }
    // 3. every cut
    {
        Built b;
        build(n, &b);
        for (int k = 0; k <= b.n_sub; ++k) {
            const bool ends_on_ca = k > 0 && b.subs[k - 1].kind == DRN_SUB_CA;
            build(n, &b);                                // (same arenas in the same order: the same addresses)
            const int rc1 = drn_dit_forward_range(&b.a, 0, k, DRN_DIT_EMBED, STREAM);
            const std::vector<rec::Launch> one = rec::launches();
            ++cut_cases;
            if (ends_on_ca) {
                if (rc1 != DRN_EINVAL || !one.empty()) fail(name + ": a part that ends on a cross-attention sub-block is not refused, cut " + std::to_string(k));
                continue;
            }
            if (rc1 != DRN_OK) fail(name + ": part (EMBED, 0.." + std::to_string(k) + ") returns " + std::to_string(rc1));
            std::string bad = rec::check_call();
            build(n, &b);
            const int rc2 = drn_dit_forward_range(&b.a, k, b.n_sub, DRN_DIT_FINAL, STREAM);
            if (rc2 != DRN_OK) fail(name + ": part (" + std::to_string(k) + "..n, FINAL) returns " + std::to_string(rc2));
            if (bad.empty()) bad = rec::check_call();
            if (!bad.empty()) fail(name + ": cut " + std::to_string(k) + ": " + bad);
            compare_cut(name + ": cut " + std::to_string(k), whole, one, rec::launches(), &cut_substitutions);
        }
        case_line(name + ": every cut", "OK    ", whole.size());
    }
    // 5. an injected failure at every launch
    if (inject) {
        for (size_t k = 0; k < whole.size(); ++k) {
            Built b;
            build(n, &b);
            rec::fail_launch((int)k, 700 + (int)(k % 100));
            const int rc = drn_dit_forward(&b.a, STREAM);
            if (rc != 700 + (int)(k % 100)) fail(name + ": launch " + std::to_string(k) + " failed with " + std::to_string(700 + (int)(k % 100)) + ", the call returns " + std::to_string(rc));
            if (rec::launches_after_failure() != 0 || rec::launches().size() != k + 1) fail(name + ": launches after the failed launch " + std::to_string(k));
            ++tally.injected;
        }
        case_line(name + ": a failure injected at every launch", "OK    ", whole.size());
    }
}

// section B, attention: the plan tiles [0, S) and is what a self-attention sub-block launches
long plan_sizes = 0;
void attention_plan_is_launched(int heads, int64_t S) {
    int64_t* plan = new int64_t[6];                          // exactly what the entry may write
    const int np = drn_attention_plan(heads, S, S, plan);
    const std::string name = "attention plan heads " + std::to_string(heads) + " S " + std::to_string(S);
    if (np < 1 || np > 2 || plan[0] != 0 || plan[3 * np - 2] != S || (np == 2 && (plan[1] != plan[3] || plan[1] <= 0 || plan[1] >= S)))
        fail(name + ": the ranges do not tile [0, S)");
    Net n{(int64_t)heads * 128, (int64_t)heads * 512, 1, heads, S, 2};
    n.kinds = "f";
    Built b;
    build(n, &b);
    if (drn_dit_forward(&b.a, STREAM) != DRN_OK) fail(name + ": the forward is refused");
    const std::string bad = rec::check_call();
    if (!bad.empty()) fail(name + ": " + bad);
    std::vector<rec::Launch> att;
    int combines = 0;
    for (const rec::Launch& l : rec::launches()) {
        if (has(l, "attention") && has(l, "fwd_kernel")) att.push_back(l);
        if (has(l, "combine")) ++combines;
    }
    if ((int)att.size() != np) fail(name + ": the plan has " + std::to_string(np) + " launches, the forward makes " + std::to_string(att.size()));
    int want_combines = 0;
    for (int p = 0; p < np; ++p) {
        const int64_t q0 = plan[3 * p], nq = plan[3 * p + 1] - q0, ns = plan[3 * p + 2], D = n.D;
        if (att[p].ptrs[0] != (uintptr_t)b.a.QKV + (uintptr_t)(q0 * 3 * D * 2) || att[p].ptrs[3] != (uintptr_t)b.a.O + (uintptr_t)(q0 * D * 2))
            fail(name + ": launch " + std::to_string(p) + " does not start at query " + std::to_string(q0));
        const int64_t per = (nq + 255) / 256 * heads * n.B, chunk = ((S + ns - 1) / ns + 63) / 64 * 64, chunks = ns > 1 ? (S + chunk - 1) / chunk : 1;
        if ((int64_t)att[p].grid[0] != per * chunks) fail(name + ": launch " + std::to_string(p) + " has " + std::to_string(att[p].grid[0]) + " workgroups, the plan says " + std::to_string(per * chunks));
        want_combines += ns > 1;
    }
    if (combines != want_combines) fail(name + ": combine launches");
    delete[] plan;
    ++plan_sizes;
}

}  // namespace

void family_forward() {
    begin_entry("drn_dit_forward");
    begin_entry("drn_dit_forward_range");
    if (list_only) return;

    // the tiny nets of the GPU tests, and the full model at 256 and 18 432 tokens
    const Net shapes[] = {{256, 1024, 2, 2, 128, 1}, {256, 1024, 2, 2, 128, 3}, {2048, 8192, 2, 16, 256, 1}, {4096, 16384, 28, 32, 256, 1}, {4096, 16384, 28, 32, 18432, 1}};
    for (int s = 0; s < 5; ++s) {
        const int modes[6][3] = {{0, 0, 0}, {0, 0, 1}, {1, 0, 0}, {1, 0, 1}, {1, 1, 0}, {1, 1, 1}};      // precision, mx_fused, attn_precision
        for (const auto& m : modes) {
            Net n = shapes[s];
            n.precision = m[0], n.mx_fused = m[1], n.attn_precision = m[2];
            walk_net(n, /*inject=*/s <= 2);
        }
    }
    // MXFP8 attention below its 2048-token rule: forced on, so the small nets walk those launches too
    drn_attention_mxfp8_force(forced_attmx = 1);
    for (int s = 0; s < 3; ++s) {
        Net n = shapes[s];
        n.attn_precision = 1;
        walk_net(n, true);
        n.precision = 1, n.mx_fused = 1;
        walk_net(n, true);
    }
    drn_attention_mxfp8_force(forced_attmx = 0);
    // the 32x32x16 attention body: an mx_fused forward keeps bf16 O and the quantise launch at that site
    drn_attention_force_shape16(forced_body16 = 0);
    {
        Net n = shapes[2];
        n.precision = 1, n.mx_fused = 1;
        walk_net(n, true);
    }
    drn_attention_force_shape16(-1);
    forced_body16 = 1;
    // shapes whose attention plan has a split-KV launch (the token bands of sequence parallelism, a fractional last round):
    // the attn_ws carve, its sizer and the combine launches
    for (const Net& shape : {Net{2048, 8192, 2, 16, 2304, 2}, Net{4096, 16384, 2, 32, 2304, 1}, Net{2048, 8192, 1, 16, 4817, 3}, Net{512, 2048, 2, 4, 9000, 1}}) {
        const int modes[4][3] = {{0, 0, 0}, {1, 1, 0}, {0, 0, 1}, {1, 1, 1}};
        for (const auto& m : modes) {
            Net n = shape;
            n.precision = m[0], n.mx_fused = m[1], n.attn_precision = m[2];
            walk_net(n, n.S == 2304 && n.B == 2);
        }
    }
    if (!nets_with_attn_ws) fail("no walked forward needs attn_ws: the split-KV carve is not covered");
    // other sub-block orders: two cross-attentions in a row, no attention at all, no sub-block
    for (const char* kinds : {"fccm", "cm", "mf", "c"}) {
        Net n = shapes[2];
        n.kinds = kinds;
        walk_net(n, true);
        n.precision = 1, n.mx_fused = 1;
        walk_net(n, false);
    }
    {
        Net n = shapes[0];
        n.L = 0;
        walk_net(n, true);
        n = shapes[0], n.with_timer = true;
        expect_ok("forward " + net_name(n) + ": with a timer", [&] { return forward(n); });
    }
    printf("forward cuts %ld deferred-sum substitutions at a cut %ld launches %ld\n", cut_cases, cut_substitutions, forward_launches);

    // 6. and the argument block's refusals, one at a time
    const Net base = shapes[2];
    struct ArgChange { const char* what; std::function<void(drn_dit_forward_args&)> apply; };
    const ArgChange changes[] = {
        {"struct_bytes + 8", [](drn_dit_forward_args& a) { a.struct_bytes += 8; }}, {"struct_bytes - 8", [](drn_dit_forward_args& a) { a.struct_bytes -= 8; }},
        {"struct_bytes 0", [](drn_dit_forward_args& a) { a.struct_bytes = 0; }}, {"S 0", [](drn_dit_forward_args& a) { a.S = 0; }}, {"B 0", [](drn_dit_forward_args& a) { a.B = 0; }},
        {"D != heads 128", [](drn_dit_forward_args& a) { a.heads = 15; }}, {"hidden 0", [](drn_dit_forward_args& a) { a.hidden = 0; }}, {"n_sub < 0", [](drn_dit_forward_args& a) { a.n_sub = -1; }},
        {"null subs", [](drn_dit_forward_args& a) { a.subs = nullptr; }}, {"null X", [](drn_dit_forward_args& a) { a.X = nullptr; }}, {"null H", [](drn_dit_forward_args& a) { a.H = nullptr; }},
        {"null QKV", [](drn_dit_forward_args& a) { a.QKV = nullptr; }}, {"null O", [](drn_dit_forward_args& a) { a.O = nullptr; }}, {"null U", [](drn_dit_forward_args& a) { a.U = nullptr; }},
        {"null Y", [](drn_dit_forward_args& a) { a.Y = nullptr; }}, {"null P", [](drn_dit_forward_args& a) { a.P = nullptr; }}, {"null w_patch", [](drn_dit_forward_args& a) { a.w_patch = nullptr; }},
        {"null w_final", [](drn_dit_forward_args& a) { a.w_final = nullptr; }}, {"null final_shift", [](drn_dit_forward_args& a) { a.final_shift = nullptr; }},
        {"null final_scale", [](drn_dit_forward_args& a) { a.final_scale = nullptr; }}, {"null shift", [](drn_dit_forward_args& a) { a.shift = nullptr; }},
        {"null scale", [](drn_dit_forward_args& a) { a.scale = nullptr; }}, {"null gate", [](drn_dit_forward_args& a) { a.gate = nullptr; }},
        {"precision 2", [](drn_dit_forward_args& a) { a.precision = 2; }}, {"null gemm_ws", [](drn_dit_forward_args& a) { a.gemm_ws = nullptr; }},
        {"mx_fused 1 with precision 0", [](drn_dit_forward_args& a) { a.mx_fused = 1; }}, {"mx_fused 2", [](drn_dit_forward_args& a) { a.mx_fused = 2; }},
        {"attn_precision 2", [](drn_dit_forward_args& a) { a.attn_precision = 2; }}, {"attn_precision 1 without mx_attn", [](drn_dit_forward_args& a) { a.attn_precision = 1; }},
        {"a sub-block of kind 3", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[4].kind = 3; }}, {"CA without addvec", [](drn_dit_forward_args& a) { a.addvec = nullptr; }},
        {"CA with ca_index < 0", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[1].ca_index = -1; }}, {"FA without w_a", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[3].w_a = nullptr; }},
        {"MLP without w_b", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[5].w_b = nullptr; }}, {"FA without qn", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[0].qn = nullptr; }},
        {"FA without kn", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[0].kn = nullptr; }}, {"FA without cos", [](drn_dit_forward_args& a) { a.cos = nullptr; }},
        {"FA without sin", [](drn_dit_forward_args& a) { a.sin = nullptr; }},
        // what a launcher further down would refuse only after the launches in front of it: the header promises the check up front
        {"kpad % 64", [](drn_dit_forward_args& a) { a.kpad = 200; }}, {"n_final % 128", [](drn_dit_forward_args& a) { a.n_final = 64; }},
        {"hidden % 128", [](drn_dit_forward_args& a) { a.hidden = 8192 + 64; }}, {"D > 8192", [](drn_dit_forward_args& a) { a.heads = 65, a.D = 65 * 128; }},
        {"QKV off 16 bytes", [](drn_dit_forward_args& a) { a.QKV = (char*)a.QKV + 8; }}, {"O off 16 bytes", [](drn_dit_forward_args& a) { a.O = (char*)a.O + 8; }},
        {"Y off 16 bytes", [](drn_dit_forward_args& a) { a.Y = (char*)a.Y + 8; }}, {"H off 16 bytes", [](drn_dit_forward_args& a) { a.H = (char*)a.H + 8; }},
        {"P off 16 bytes", [](drn_dit_forward_args& a) { a.P = (const char*)a.P + 8; }}, {"w_patch off 16 bytes", [](drn_dit_forward_args& a) { a.w_patch = (const char*)a.w_patch + 8; }},
        {"w_final off 16 bytes", [](drn_dit_forward_args& a) { a.w_final = (const char*)a.w_final + 8; }}, {"X off 16 bytes", [](drn_dit_forward_args& a) { a.X = (char*)a.X + 8; }},
        {"U off 16 bytes", [](drn_dit_forward_args& a) { a.U = (char*)a.U + 8; }}, {"gemm_ws off 16 bytes", [](drn_dit_forward_args& a) { a.gemm_ws = (char*)a.gemm_ws + 8; }},
        {"w_a of a sub-block off 16 bytes", [](drn_dit_forward_args& a) { drn_dit_sub& e = ((drn_dit_sub*)a.subs)[3]; e.w_a = (const char*)e.w_a + 8; }},
        {"w_b of a sub-block off 16 bytes", [](drn_dit_forward_args& a) { drn_dit_sub& e = ((drn_dit_sub*)a.subs)[5]; e.w_b = (const char*)e.w_b + 8; }},
    };
    for (const ArgChange& c : changes)
        for (int range = 0; range < 2; ++range)
            expect_refusal(std::string(range ? "drn_dit_forward_range: " : "drn_dit_forward: ") + c.what, [&] {
                Built b;
                build(base, &b);
                c.apply(b.a);
                return range ? drn_dit_forward_range(&b.a, 0, 0, DRN_DIT_FINAL, STREAM) : drn_dit_forward(&b.a, STREAM);
            });
    expect_refusal("drn_dit_forward: null args", [] { rec::reset(); return drn_dit_forward(nullptr, STREAM); });
    expect_refusal("drn_dit_forward_range: null args", [] { rec::reset(); return drn_dit_forward_range(nullptr, 0, 0, 3, STREAM); });
    {
        Net mxn = base;
        mxn.precision = 1, mxn.mx_fused = 1, mxn.attn_precision = 1;
        const ArgChange mxc[] = {{"precision 1 without AQ", [](drn_dit_forward_args& a) { a.AQ = nullptr; }}, {"precision 1 without AS", [](drn_dit_forward_args& a) { a.AS = nullptr; }},
                                 {"mx_fused without UQ", [](drn_dit_forward_args& a) { a.UQ = nullptr; }}, {"mx_fused without US", [](drn_dit_forward_args& a) { a.US = nullptr; }},
                                 {"precision 1 without s_a", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[0].s_a = nullptr; }},
                                 {"precision 1 without s_b", [](drn_dit_forward_args& a) { ((drn_dit_sub*)a.subs)[2].s_b = nullptr; }},
                                 {"precision 1 with hidden % 256", [](drn_dit_forward_args& a) { a.hidden = 8192 + 128; }},
                                 {"mx_attn off 256 bytes", [](drn_dit_forward_args& a) { a.mx_attn = (char*)a.mx_attn + 128; }},
                                 {"AQ off 16 bytes", [](drn_dit_forward_args& a) { a.AQ = (char*)a.AQ + 8; }}, {"AS off 4 bytes", [](drn_dit_forward_args& a) { a.AS = (char*)a.AS + 2; }},
                                 {"UQ off 16 bytes", [](drn_dit_forward_args& a) { a.UQ = (char*)a.UQ + 8; }}, {"US off 4 bytes", [](drn_dit_forward_args& a) { a.US = (char*)a.US + 2; }},
                                 {"s_a of a sub-block off 4 bytes", [](drn_dit_forward_args& a) { drn_dit_sub& e = ((drn_dit_sub*)a.subs)[0]; e.s_a = (const char*)e.s_a + 2; }},
                                 {"s_b of a sub-block off 4 bytes", [](drn_dit_forward_args& a) { drn_dit_sub& e = ((drn_dit_sub*)a.subs)[2]; e.s_b = (const char*)e.s_b + 2; }}};
        for (const ArgChange& c : mxc)
            expect_refusal(std::string("drn_dit_forward: ") + c.what, [&] {
                Built b;
                build(mxn, &b);
                c.apply(b.a);
                return drn_dit_forward(&b.a, STREAM);
            });
    }
    {
        // attn_ws off 16 bytes, on a net whose plan has a split-KV launch (the base net needs no attn_ws)
        const Net split{2048, 8192, 2, 16, 2304, 2};
        expect_refusal("drn_dit_forward: attn_ws off 16 bytes", [&] {
            Built b;
            build(split, &b);
            if (!b.a.attn_ws) fail("the net chosen for the attn_ws case needs no attn_ws");
            b.a.attn_ws = (char*)b.a.attn_ws + 8;
            return drn_dit_forward(&b.a, STREAM);
        });
        // the row limits, each with the largest size that is still taken beside it: B <= 65535 holds with a self-attention sub-block
        // only, B S < 2^31 always (one-head nets, fake arenas: X alone is 2^39 bytes)
        Net fa{128, 128, 1, 1, 1, 65535};
        fa.kinds = "f", fa.kpad = 64;
        expect_ok("drn_dit_forward: B 65535 with a FA sub-block", [&] { return forward(fa); });
        fa.B = 65536;
        expect_refusal("drn_dit_forward: B 65536 with a FA sub-block", [&] { return forward(fa); });
        fa.kinds = "m";
        expect_ok("drn_dit_forward: B 65536 without a FA sub-block", [&] { return forward(fa); });
        Net rows{128, 128, 1, 1, 32768, 65535};
        rows.kinds = "m", rows.kpad = 64;
        expect_ok("drn_dit_forward: B S == 2^31 - 32768", [&] { return forward(rows); });
        rows.B = 65536;
        expect_refusal("drn_dit_forward: B S == 2^31", [&] { return forward(rows); });
    }
    const int n_sub = base.L * 3;
    struct RangeCase { const char* what; int lo, hi, flags; bool ok; };
    const RangeCase ranges[] = {{"sub_lo < 0", -1, 2, 3, false}, {"sub_lo > sub_hi", 3, 2, 3, false}, {"sub_hi > n_sub", 0, n_sub + 1, 3, false}, {"flags 4", 0, n_sub, 4, false},
                                {"flags 7", 0, n_sub, 7, false}, {"flags -1", 0, n_sub, -1, false}, {"a part without FINAL that ends on a cross-attention", 0, 2, 1, false},
                                {"the final layer alone", n_sub, n_sub, DRN_DIT_FINAL, true}, {"the patch embed alone", 0, 0, DRN_DIT_EMBED, true},
                                {"one sub-block, no flag", 2, 3, 0, true}, {"the whole forward", 0, n_sub, 3, true}, {"a part with FINAL that ends on a cross-attention", 0, 2, 3, true}};
    for (const RangeCase& r : ranges) {
        auto call = [&] {
            Built b;
            build(base, &b);
            return drn_dit_forward_range(&b.a, r.lo, r.hi, r.flags, STREAM);
        };
        if (r.ok) expect_ok(std::string("drn_dit_forward_range: ") + r.what, call);
        else expect_refusal(std::string("drn_dit_forward_range: ") + r.what, call);
    }

    // section B, attention: heads x a sweep of S up to 20 000 (every 256-row q-block count, and sizes around the block edges)
    for (int heads : {1, 2, 4, 16, 32})
        for (int64_t S = 1; S <= 20000; S += (S < 600 ? 37 : 509)) attention_plan_is_launched(heads, S);
    for (int heads : {1, 2, 4, 16, 32})
        for (int64_t S : {255, 256, 257, 2048, 2304, 4096, 8191, 8192, 8193, 18432, 20000}) attention_plan_is_launched(heads, S);
    printf("attention plans walked %ld\n", plan_sizes);
}

}  // namespace hw
