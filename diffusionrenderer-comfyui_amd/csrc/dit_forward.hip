// drn_dit_forward: the launch sequence of one CleanGeneralDIT forward on one GPU, enqueued by ONE call.
//
// Replaces the Python-level block loop of the reference (CleanGeneralDIT.py:686-706: patch embed, 28 x {FA, CA, MLP}, final
// layer) as a SEQUENCER only: every launch below is one of the kernels behind the other entry points of drn.h, called with the
// arguments the per-launch host path (dit_engine.HipDiT._run) passes, in the same order - results are bit-identical to it,
// in both precisions of the block linears (args->precision: 0 = bf16, 1 = MXFP8 with the activations quantised per linear).
// Why it exists: a forward is ~570 launches; through ctypes + torch wrappers each costs the host 6-12 us, which at S = 256
// (cfg 1: a 6.8 ms GPU step) made the host the bound of the denoising loop.  From C the same launches cost the host ~2 ms.
// Host code only (no kernel lives in this file).
#include "drn_common.h"
#include "drn_launchers.h"

// ---- how to cover the (q-block, head) grid with whole rounds of the 256 CUs (was native.attention_plan; measured cost model)
static const int kCUs = 256;

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static int pick_kv_splits(int64_t batch, int64_t heads, int64_t Sq, int64_t Sk, double* cost_out) {
    const int64_t blocks = batch * heads * ((Sq + 255) / 256);
    int best = 1;
    double best_cost = (double)ceil_div(blocks, kCUs);
    const int cand[3] = {2, 4, 8};
    for (int i = 0; i < 3; ++i) {
        const int n = cand[i];
        if (Sk / n < 512) break;
        // ~4 % of an unsplit workgroup per extra workgroup (prologue, fp32 partial store) and ~6 % for the combine pass
        const double cost = (double)ceil_div(blocks * n, kCUs) * (1.0 / n + 0.04) + 0.06;
        const double lim = (double)ceil_div(blocks, kCUs) * 0.93;
        if (cost < (best_cost < lim ? best_cost : lim)) {
            best = n;
            best_cost = cost;
        }
    }
    if (cost_out) *cost_out = best_cost;
    return best;
}

// plan[3 * i + {0, 1, 2}] = (q_begin, q_end, kv_splits); returns the number of launches (1 or 2)
extern "C" int drn_attention_plan(int heads, int64_t Sq, int64_t Sk, int64_t* plan) {
    if (heads <= 0 || Sq <= 0 || Sk <= 0 || !plan) return 0;
    const int64_t per_qb = heads;                       // the plan of ONE clip (batch-invariant summation order)
    const int64_t nqb = (Sq + 255) / 256;
    const int64_t blocks = nqb * per_qb;
    const int n_all = pick_kv_splits(1, heads, Sq, Sk, nullptr);
    const double cost_all = n_all == 1 ? (double)ceil_div(blocks, kCUs)
                                       : (double)ceil_div(blocks * n_all, kCUs) * (1.0 / n_all + 0.04) + 0.06;
    const int64_t rounds = blocks / kCUs;
    const int64_t nqb_main = (rounds * kCUs) / per_qb;
    plan[0] = 0; plan[1] = Sq; plan[2] = n_all;
    if (rounds == 0 || nqb_main == 0 || nqb_main == nqb) return 1;
    const int64_t q_cut = nqb_main * 256;
    const int n_tail = pick_kv_splits(1, heads, Sq - q_cut, Sk, nullptr);
    const int64_t tail_blocks = (nqb - nqb_main) * per_qb;
    const double cost_tail = n_tail == 1 ? (double)ceil_div(tail_blocks, kCUs)
                                         : (double)ceil_div(tail_blocks * n_tail, kCUs) * (1.0 / n_tail + 0.04) + 0.06;
    const double cost_two = (double)ceil_div(nqb_main * per_qb, kCUs) + cost_tail + 0.02;      // + the launch boundary
    if (cost_two < cost_all) {
        plan[0] = 0; plan[1] = q_cut; plan[2] = 1;
        plan[3] = q_cut; plan[4] = Sq; plan[5] = n_tail;
        return 2;
    }
    return 1;
}

// ---- optional per-launch timing (bench.py's roofline leg): HIP event pairs around every `sample_every`-th GEMM / attention
struct drn_timer {
    int capacity, used, sample_every;
    int seen[2];                                        // launches seen per kind (0 = gemm, 1 = attention)
    hipEvent_t* ev;                                     // 2 per record
    int* kind;
    double* flops;
    double* bytes;
};

extern "C" void* drn_timer_create(int capacity, int sample_every) {
    if (capacity <= 0) return nullptr;
    drn_timer* t = new drn_timer();
    t->capacity = capacity;
    t->used = 0;
    t->sample_every = sample_every > 0 ? sample_every : 1;
    t->seen[0] = t->seen[1] = 0;
    t->ev = new hipEvent_t[2 * (size_t)capacity];
    t->kind = new int[capacity];
    t->flops = new double[capacity];
    t->bytes = new double[capacity];
    for (int i = 0; i < 2 * capacity; ++i)
        if (hipEventCreate(&t->ev[i]) != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipEventDestroy(t->ev[j]);
            delete[] t->ev; delete[] t->kind; delete[] t->flops; delete[] t->bytes;
            delete t;
            return nullptr;
        }
    return t;
}

extern "C" void drn_timer_destroy(void* h) {
    drn_timer* t = (drn_timer*)h;
    if (!t) return;
    for (int i = 0; i < 2 * t->capacity; ++i) (void)hipEventDestroy(t->ev[i]);
    delete[] t->ev; delete[] t->kind; delete[] t->flops; delete[] t->bytes;
    delete t;
}

extern "C" int drn_timer_count(void* h) { return h ? ((drn_timer*)h)->used : 0; }
extern "C" int drn_timer_seen(void* h, int kind) { return (h && (kind == 0 || kind == 1)) ? ((drn_timer*)h)->seen[kind] : 0; }

// record i after the stream has been synchronised: kind, milliseconds, algorithmic FLOPs and bytes of that launch
extern "C" int drn_timer_read(void* h, int i, int* kind, float* ms, double* flops, double* bytes) {
    drn_timer* t = (drn_timer*)h;
    if (!t || i < 0 || i >= t->used) return DRN_EINVAL;
    const hipError_t e = hipEventElapsedTime(ms, t->ev[2 * i], t->ev[2 * i + 1]);
    if (e != hipSuccess) return (int)e;
    *kind = t->kind[i];
    *flops = t->flops[i];
    *bytes = t->bytes[i];
    return DRN_OK;
}

namespace {
struct Scope {                                           // event pair around one sampled launch
    drn_timer* t;
    int slot;
    hipStream_t st;
    Scope(drn_timer* timer, int kind, double flops, double bytes, hipStream_t stream) : t(timer), slot(-1), st(stream) {
        if (!t) return;
        const int c = t->seen[kind]++;
        if (c % t->sample_every != 0 || t->used >= t->capacity) return;
        slot = t->used++;
        t->kind[slot] = kind;
        t->flops[slot] = flops;
        t->bytes[slot] = bytes;
        (void)hipEventRecord(t->ev[2 * slot], st);
    }
    ~Scope() {
        if (slot >= 0) (void)hipEventRecord(t->ev[2 * slot + 1], st);
    }
};
}  // namespace

extern "C" int64_t drn_dit_forward_attn_workspace_bytes(int64_t B, int heads, int64_t S) {
    int64_t plan[6];
    const int n = drn_attention_plan(heads, S, S, plan);
    int64_t need = 0;
    for (int i = 0; i < n; ++i)
        if (plan[3 * i + 2] > 1) {
            const int64_t b = drn_attention_splitkv_workspace_bytes((int)B, heads, plan[3 * i + 1] - plan[3 * i], (int)plan[3 * i + 2]);
            need = b > need ? b : need;
        }
    return need;
}

// the fp32 slices of one bf16 linear [B S, N, K] (0 when it is not split)
static int64_t bf16_splitk_bytes(int64_t B, int64_t S, int64_t N, int64_t K) {
    return drn_gemm_splitk_workspace_bytes(B * S, N, S <= 1024 ? drn_gemm_splitk_choice(S, N, K) : 1);
}

extern "C" int64_t drn_dit_forward_gemm_workspace_bytes(int64_t B, int64_t S, int64_t D, int64_t hidden, int64_t n_final, int64_t kpad) {
    const int64_t shapes[6][2] = {{D, kpad}, {3 * D, D}, {D, D}, {hidden, D}, {D, hidden}, {n_final, D}};
    int64_t need = 0;
    for (int i = 0; i < 6; ++i) {
        const int64_t b = bf16_splitk_bytes(B, S, shapes[i][0], shapes[i][1]);
        need = b > need ? b : need;
    }
    return need;
}

extern "C" int64_t drn_dit_forward_mx_act_bytes(int64_t B, int64_t S, int64_t D, int64_t hidden) {
    const int64_t k = D > hidden ? D : hidden;
    return B * S * k + B * S * (k / 32);
}

extern "C" int64_t drn_dit_forward_mx_u_bytes(int64_t B, int64_t S, int64_t hidden) {
    return B * S * hidden + B * S * (hidden / 32);
}

// the MXFP8 attention scratch: QQ | KQ | VT | QS | KS | VS, each rounded up to 256 bytes (drn.h): the ONE statement of the layout;
// out = the six byte offsets in that order, the total, Sp
extern "C" int drn_dit_forward_mx_attn_layout(int64_t B, int64_t S, int64_t D, int64_t* out) {
    DRN_CHECK_ARG(out && B > 0 && S > 0 && D > 0 && D % 128 == 0);
    const int64_t Sp = (S + 127) / 128 * 128;
    const int64_t bytes[6] = {B * S * D, B * S * D, B * D * Sp, B * S * (D / 32), B * S * (D / 32), B * D * (Sp / 32)};
    int64_t o = 0;
    for (int i = 0; i < 6; ++i) {
        out[i] = o;
        o += (bytes[i] + 255) / 256 * 256;
    }
    out[6] = o;
    out[7] = Sp;
    return DRN_OK;
}

extern "C" int64_t drn_dit_forward_mx_attn_bytes(int64_t B, int64_t S, int64_t D) {
    int64_t l[8];
    return drn_dit_forward_mx_attn_layout(B, S, D, l) == DRN_OK ? l[6] : 0;
}

extern "C" int64_t drn_dit_forward_mx_gemm_workspace_bytes(int64_t B, int64_t S, int64_t D, int64_t hidden) {
    const int64_t M = B * S;
    const int64_t shapes[4][2] = {{3 * D, D}, {D, D}, {hidden, D}, {D, hidden}};
    int64_t need = 0;
    for (int i = 0; i < 4; ++i) {
        const int splits = drn_gemm_mxfp8_splitk_choice(S, shapes[i][0], shapes[i][1]);
        const int64_t b = drn_gemm_splitk_workspace_bytes(M, shapes[i][0], splits);
        need = b > need ? b : need;
    }
    return need;
}

extern "C" int64_t drn_dit_forward_args_bytes(void) { return (int64_t)sizeof(drn_dit_forward_args); }
extern "C" int64_t drn_dit_sub_bytes(void) { return (int64_t)sizeof(drn_dit_sub); }

// ---- the sequencer
// launch decisions that change a summation order come from the rows of ONE clip (batch-invariant results): rows_per_batch where
// M is whole clips of it, else M
static int64_t clip_rows(int64_t M, int64_t rows_per_batch) {
    return (rows_per_batch > 0 && rows_per_batch < M && M % rows_per_batch == 0) ? rows_per_batch : M;
}

namespace {
struct MxPtr {                                           // an MXFP8 matrix: elements | scales (q == NULL: none)
    void* q;
    void* s;
};

// C [M, N] = epi(A [M, K] . W [N, K]^T), every operand contiguous (lda = K, ldc = ldr = N).  Filled by name at the call sites
// (designated initialisers); a field left out is NULL / false
struct Linear {
    const void* a;                                       // A as bf16 ...
    MxPtr a_mx;                                          // ... or (precision 1) written as MX by its producer already: `a` is not read
    const void* w;
    const void* sw;                                      // precision 1: the E8M0 scales of w
    void* c;                                             // C as bf16 ...
    MxPtr c_mx;                                          // ... or (MLP-up of an mx_fused forward) as MX, where that entry has a kernel
    int64_t M, N, K;
    int epi;
    const void* gate;
    const void* residual;
    // a split-K product with the gated-residual epilogue may stop after its slices: the next LayerNorm pass folds sum + epilogue
    // in (drn_splitk_gate_res_ln_modulate: the same bits).  The per-launch host path never defers; the tests compare the two.
    bool may_defer;
};

struct Forward {
    const drn_dit_forward_args* a;
    void* stream;
    int64_t M;                                           // B S rows
    int64_t al[8];                                       // attn_precision 1: drn_dit_forward_mx_attn_layout
    const bf16_t* pending;                               // the broadcast cross-attention residual not yet added to X
    int deferred;                                        // > 0: X still lacks sum(partials) + gate/residual of the last linear
    const bf16_t* deferred_gate;

    drn_timer* timer() const { return (drn_timer*)a->timer; }
    bool defers(const Linear& l) const {
        return l.may_defer && l.epi == DRN_EPI_GATE_RES && l.N == a->D && l.N > 1024 && l.residual == l.c;
    }

    // LayerNorm + modulate of X into H, folding a deferred split-K epilogue in.  mx_out (mx_fused, in front of a FA / MLP
    // sub-block): the result goes to AQ | AS as MXFP8 [M, D] instead (H is not written): the q|k|v / MLP-up linear reads it there.
    int ln_next(const bf16_t* shift, const bf16_t* scale, bool mx_out) {
        const int64_t D = a->D, S = a->S;
        int rc;
        if (deferred && mx_out)
            rc = drn_splitk_gate_res_ln_modulate_mx(a->gemm_ws, deferred, a->X, deferred_gate, pending, shift, scale, nullptr, a->AQ,
                                                    a->AS, M, D, S, a->eps, stream);
        else if (deferred)
            rc = drn_splitk_gate_res_ln_modulate(a->gemm_ws, deferred, a->X, deferred_gate, pending, shift, scale, a->H, M, D, S, a->eps,
                                                 stream);
        else if (mx_out)
            rc = drn_ln_modulate_mx(a->X, pending, shift, scale, nullptr, a->AQ, a->AS, M, D, S, a->eps, stream);
        else
            rc = drn_ln_modulate(a->X, pending, shift, scale, a->H, M, D, S, a->eps, stream);
        deferred = 0;
        pending = nullptr;
        return rc;
    }

    // out = epi(A . W^T) exactly as native.gemm dispatches it: split-K for few-token products
    int linear_bf16(const Linear& l) {
        const int64_t M = l.M, N = l.N, K = l.K, rpb = a->S, ldr = l.residual ? N : 0;
        const int64_t Mb = clip_rows(M, rpb);
        const int splits = Mb <= 1024 ? drn_gemm_splitk_choice(Mb, N, K) : 1;
        Scope sc(timer(), 0, 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N * (l.residual ? 2 : 1)), (hipStream_t)stream);
        if (splits > 1 && defers(l)) {
            deferred = splits;
            deferred_gate = (const bf16_t*)l.gate;
            return drn_gemm_bf16_splitk_partials(l.a, l.w, M, N, K, K, K, rpb, splits, a->gemm_ws, stream);
        }
        if (splits > 1)
            return drn_gemm_bf16_splitk(l.a, l.w, l.c, M, N, K, K, K, N, l.epi, l.gate, l.residual, ldr, rpb, splits, a->gemm_ws, stream);
        // QKV and MLP-up of a clip of 18 432 tokens at D = 4096: 13.5 and 18 rounds of 256 x 256 tiles are 9 and 12 whole rounds of
        // 384 x 256 ones, measured in this sequence 1.318 -> 1.280 and 1.753 -> 1.736 ms, the step 269.32 -> 265.24 ms
        // (profiles/harvest_18k.txt 1, 2); same bits.  Out-proj ties and keeps its plan.
        if (Mb == 18432 && K == 4096 && ((N == 12288 && l.epi == DRN_EPI_NONE) || (N == 16384 && l.epi == DRN_EPI_GELU)))
            return drn_gemm_bf16_measured384(l.a, l.w, l.c, M, N, K, K, K, N, l.epi, l.gate, l.residual, ldr, rpb, stream);
        return drn_gemm_bf16(l.a, l.w, l.c, M, N, K, K, K, N, l.epi, l.gate, l.residual, ldr, rpb, stream);
    }

    // The same for a block linear of a precision-1 (MXFP8) forward: quantise A into AQ | AS unless its producer wrote it as MX,
    // then the MXFP8 product chosen as native.gemm_mxfp8 chooses it (drn_gemm_mxfp8_splitk_choice): drn_gemm_mxfp8 (0), the fused
    // few-token kernel (1) or its K slices (> 1).  With c_mx the GELU result leaves as MX through drn_gemm_mxfp8_gelu_mx where that
    // entry has a kernel (*c_is_mx = true), else as bf16 into c (the consumer quantises by launch, the same bytes).
    int linear_mx(const Linear& l, bool* c_is_mx) {
        const int64_t M = l.M, N = l.N, K = l.K, rpb = a->S, ldr = l.residual ? N : 0;
        MxPtr A = l.a_mx;
        if (!A.q) {
            DRN_TRY(drn_mx_quant_bf16(l.a, M, K, K, a->AQ, a->AS, stream));
            A = {a->AQ, a->AS};
        }
        const int splits = drn_gemm_mxfp8_splitk_choice(clip_rows(M, rpb), N, K);
        Scope sc(timer(), 0, 2.0 * M * N * K, 1.03 * (M * K + N * K) + 2.0 * M * N * (l.residual ? 2 : 1), (hipStream_t)stream);
        if (c_is_mx) *c_is_mx = l.c_mx.q && l.epi == DRN_EPI_GELU && splits <= 1;
        if (c_is_mx && *c_is_mx) return drn_gemm_mxfp8_gelu_mx(A.q, A.s, l.w, l.sw, l.c_mx.q, l.c_mx.s, M, N, K, rpb, stream);
        if (splits == 0) return drn_gemm_mxfp8(A.q, A.s, l.w, l.sw, l.c, M, N, K, N, l.epi, l.gate, l.residual, ldr, rpb, stream);
        if (splits > 1 && defers(l)) {
            deferred = splits;
            deferred_gate = (const bf16_t*)l.gate;
            return drn_gemm_mxfp8_splitk_partials(A.q, A.s, l.w, l.sw, M, N, K, rpb, splits, a->gemm_ws, stream);
        }
        return drn_gemm_mxfp8_splitk(A.q, A.s, l.w, l.sw, l.c, M, N, K, N, l.epi, l.gate, l.residual, ldr, rpb, splits, a->gemm_ws, stream);
    }

    // a block linear in the precision of the forward
    int linear(const Linear& l, bool* c_is_mx = nullptr) { return a->precision == 1 ? linear_mx(l, c_is_mx) : linear_bf16(l); }

    // The self-attention of a sub-block on q | k | v in QKV (row stride 3D): norm + RoPE, then ONE walk of the plan.
    // mx_ops: MXFP8 attention - q and k leave norm + RoPE as MX, v is transposed and quantised along the keys (all into mx_attn),
    // then the block-scaled kernels; else the bf16 kernels on QKV.  o_mx: the output goes to AQ | AS as MX (O is not written; the
    // q|k|v GEMM that read them has finished in stream order), else to O as bf16.  Split keys: the same partials and combine pass.
    int self_attention(const drn_dit_sub* sb, bool mx_ops, bool o_mx) {
        const int64_t S = a->S, D = a->D, ld = 3 * D, bs = S * 3 * D;
        const int B = (int)a->B, heads = a->heads;
        const float sm_scale = (float)(1.0 / sqrt(128.0));      // the double -> float conversion of the host wrapper (native.attention)
        bf16_t* q = (bf16_t*)a->QKV;
        bf16_t* k = q + D;
        bf16_t* v = q + 2 * D;
        uint8_t *mxa = nullptr, *kq = nullptr, *vt = nullptr, *ks = nullptr, *vs = nullptr;      // MX operands: mx_ops only
        if (mx_ops) {
            mxa = (uint8_t*)a->mx_attn;
            kq = mxa + al[1], vt = mxa + al[2], ks = mxa + al[4], vs = mxa + al[5];
            DRN_TRY(drn_qk_norm_rope_mx(q, k, sb->qn, sb->kn, a->cos, a->sin, mxa + al[0], mxa + al[3], kq, ks, M, heads, ld, ld, S, 0,
                                        a->eps, 0, stream));
            DRN_TRY(drn_mx_quant_vt(v, vt, vs, B, heads, S, ld, bs, stream));
        } else {
            DRN_TRY(drn_qk_norm_rope(q, k, sb->qn, sb->kn, a->cos, a->sin, M, heads, ld, ld, S, 0, a->eps, stream));
        }
        Scope sc(timer(), 1, 4.0 * B * heads * S * S * 128, (mx_ops ? 1.0 : 2.0) * B * heads * 128 * (4.0 * S), (hipStream_t)stream);
        int64_t plan[6];
        const int n = drn_attention_plan(heads, S, S, plan);
        for (int p = 0; p < n; ++p) {
            // a launch over the queries [q0, q0 + nq) of every clip: q, O and the MX rows advance by q0 rows
            const int64_t q0 = plan[3 * p], nq = plan[3 * p + 1] - q0;
            const int ns = (int)plan[3 * p + 2];
            bf16_t* o = o_mx ? nullptr : (bf16_t*)a->O + q0 * D;
            uint8_t* oq = o_mx ? (uint8_t*)a->AQ + q0 * D : nullptr;
            uint8_t* os = o_mx ? (uint8_t*)a->AS + q0 * (D / 32) : nullptr;
            if (mx_ops) {
                const uint8_t* qq = mxa + al[0] + q0 * D;
                const uint8_t* qs = mxa + al[3] + q0 * (D / 32);
                DRN_TRY(ns > 1 ? drn_attention_splitkv_mxfp8(qq, qs, kq, ks, vt, vs, o, oq, os, B, heads, nq, S, S, S, D, S * D, sm_scale, ns,
                                                             a->attn_ws, stream)
                               : drn_attention_mxfp8(qq, qs, kq, ks, vt, vs, o, oq, os, B, heads, nq, S, S, S, D, S * D, sm_scale, stream));
            } else if (o_mx) {
                DRN_TRY(ns > 1 ? drn_attention_splitkv_bf16_mx(q + q0 * ld, k, v, nullptr, oq, os, B, heads, nq, S, ld, ld, ld, D, bs, bs, bs,
                                                               S * D, sm_scale, ns, a->attn_ws, stream)
                               : drn_attention_bf16_mx(q + q0 * ld, k, v, nullptr, oq, os, B, heads, nq, S, ld, ld, ld, D, bs, bs, bs, S * D,
                                                       sm_scale, stream));
            } else {
                DRN_TRY(ns > 1 ? drn_attention_splitkv_bf16(q + q0 * ld, k, v, o, B, heads, nq, S, ld, ld, ld, D, bs, bs, bs, S * D, sm_scale,
                                                            ns, a->attn_ws, stream)
                               : drn_attention_bf16(q + q0 * ld, k, v, o, B, heads, nq, S, ld, ld, ld, D, bs, bs, bs, S * D, sm_scale, stream));
            }
        }
        return DRN_OK;
    }
};

// every argument and workspace check of a forward: nothing is enqueued before this returns DRN_OK
int validate(const drn_dit_forward_args* a, int64_t al[8]) {
    DRN_CHECK_ARG(a && a->struct_bytes == (int64_t)sizeof(drn_dit_forward_args));
    DRN_CHECK_ARG(a->S > 0 && a->B > 0 && a->D > 0 && a->heads > 0 && a->D == (int64_t)a->heads * 128 && a->hidden > 0);
    DRN_CHECK_ARG(a->n_sub >= 0 && (a->n_sub == 0 || a->subs) && a->X && a->H && a->QKV && a->O && a->U && a->Y);
    DRN_CHECK_ARG(a->P && a->w_patch && a->w_final && a->final_shift && a->final_scale && a->shift && a->scale && a->gate);
    const int64_t S = a->S, B = a->B, D = a->D;
    DRN_CHECK_ARG(a->precision == 0 || a->precision == 1);
    // what a launcher further down would refuse only when its turn comes, after the launches in front of it: the shapes of the
    // linears (K % 64, N % 128), the LayerNorm's width, the row count, and the 16-byte bases of every GEMM operand
    DRN_CHECK_ARG(a->kpad > 0 && a->kpad % 64 == 0 && a->n_final > 0 && a->n_final % 128 == 0 && a->hidden % 128 == 0 && D <= 8192);
    DRN_CHECK_ARG(B <= ((1ll << 31) - 1) / S);
    DRN_CHECK_ARG((((uintptr_t)a->P | (uintptr_t)a->w_patch | (uintptr_t)a->w_final | (uintptr_t)a->X | (uintptr_t)a->H | (uintptr_t)a->QKV |
                    (uintptr_t)a->O | (uintptr_t)a->U | (uintptr_t)a->Y | (uintptr_t)a->gemm_ws | (uintptr_t)a->attn_ws) & 15) == 0);
    // the split-K slices of every linear this forward runs (patch embed and final layer are bf16 in either precision)
    int64_t need = drn_dit_forward_gemm_workspace_bytes(B, S, D, a->hidden, a->n_final, a->kpad);
    if (a->precision == 1) {
        DRN_CHECK_ARG(D % 256 == 0 && a->hidden % 256 == 0 && a->AQ && a->AS);
        DRN_CHECK_ARG(((uintptr_t)a->AQ & 15) == 0 && ((uintptr_t)a->AS & 3) == 0);
        DRN_CHECK_ARG(a->act_bytes >= drn_dit_forward_mx_act_bytes(B, S, D, a->hidden));
        const int64_t ends[3] = {bf16_splitk_bytes(B, S, D, a->kpad), bf16_splitk_bytes(B, S, a->n_final, D),
                                 drn_dit_forward_mx_gemm_workspace_bytes(B, S, D, a->hidden)};
        need = ends[0];
        for (int i = 1; i < 3; ++i) need = ends[i] > need ? ends[i] : need;
    }
    DRN_CHECK_ARG(need == 0 || (a->gemm_ws && a->gemm_ws_bytes >= need));
    DRN_CHECK_ARG(a->mx_fused == 0 || (a->mx_fused == 1 && a->precision == 1));
    if (a->mx_fused)
        DRN_CHECK_ARG(a->UQ && a->US && a->u_act_bytes >= drn_dit_forward_mx_u_bytes(B, S, a->hidden) && ((uintptr_t)a->UQ & 15) == 0 &&
                      ((uintptr_t)a->US & 3) == 0);
    DRN_CHECK_ARG(a->attn_precision == 0 || a->attn_precision == 1);
    if (a->attn_precision == 1) {
        DRN_TRY(drn_dit_forward_mx_attn_layout(B, S, D, al));
        DRN_CHECK_ARG(a->mx_attn && ((uintptr_t)a->mx_attn & 255) == 0 && a->mx_attn_bytes >= al[6]);
    }
    bool any_fa = false;
    for (int i = 0; i < a->n_sub; ++i) {
        const drn_dit_sub* sb = &a->subs[i];
        DRN_CHECK_ARG(sb->kind == DRN_SUB_FA || sb->kind == DRN_SUB_CA || sb->kind == DRN_SUB_MLP);
        if (sb->kind == DRN_SUB_CA) {
            DRN_CHECK_ARG(a->addvec && sb->ca_index >= 0);
            continue;
        }
        DRN_CHECK_ARG(sb->w_a && sb->w_b && (a->precision == 0 || (sb->s_a && sb->s_b)));
        DRN_CHECK_ARG((((uintptr_t)sb->w_a | (uintptr_t)sb->w_b) & 15) == 0 && (((uintptr_t)sb->s_a | (uintptr_t)sb->s_b) & 3) == 0);
        if (sb->kind == DRN_SUB_FA) {
            DRN_CHECK_ARG(sb->qn && sb->kn && a->cos && a->sin);
            any_fa = true;
        }
    }
    if (any_fa) {                                        // the split-KV partials of the plan's split launch
        DRN_CHECK_ARG(B <= 65535);                       // (the split launches and the V^T quantiser put the clip in a grid dimension)
        const int64_t att = drn_dit_forward_attn_workspace_bytes(B, a->heads, S);
        DRN_CHECK_ARG(att == 0 || (a->attn_ws && a->attn_ws_bytes >= att));
    }
    return DRN_OK;
}
}  // namespace

// A forward in parts (drn.h): patch embed (DRN_DIT_EMBED), the sub-blocks [sub_lo, sub_hi), the final layer (DRN_DIT_FINAL) - the
// launches drn_dit_forward makes for them.  A part that does not end in the final layer leaves X complete: its last
// gated-residual linear does not defer its split-K sum (the same bits: drn_splitk_gate_res_ln_modulate), and it may not end on a
// cross-attention sub-block, whose add would still be pending.
extern "C" int drn_dit_forward_range(const drn_dit_forward_args* a, int sub_lo, int sub_hi, int flags, void* stream) {
    Forward f = {};
    DRN_TRY(validate(a, f.al));
    DRN_CHECK_ARG((flags & ~(DRN_DIT_EMBED | DRN_DIT_FINAL)) == 0);
    DRN_CHECK_ARG(0 <= sub_lo && sub_lo <= sub_hi && sub_hi <= a->n_sub);
    const bool embed = (flags & DRN_DIT_EMBED) != 0, final_layer = (flags & DRN_DIT_FINAL) != 0;
    DRN_CHECK_ARG(final_layer || sub_lo == sub_hi || a->subs[sub_hi - 1].kind != DRN_SUB_CA);
    f.a = a;
    f.stream = stream;
    const int64_t D = a->D, M = f.M = a->B * a->S;
    const bool mxf = a->mx_fused == 1;                   // producers write the quantised operand of the next block linear themselves
    const MxPtr none = {nullptr, nullptr}, act = {a->AQ, a->AS}, uact = {a->UQ, a->US};
    const MxPtr h_mx = mxf ? act : none;                 // the MX operand ln_next leaves for q|k|v / MLP-up

    // patch embedding (CleanGeneralDIT.py:386/:417): X = P . w_patch^T
    if (embed) DRN_TRY(f.linear_bf16({.a = a->P, .w = a->w_patch, .c = a->X, .M = M, .N = D, .K = a->kpad, .epi = DRN_EPI_NONE}));

    for (int i = sub_lo; i < sub_hi; ++i) {
        const drn_dit_sub* sb = &a->subs[i];
        const bool may_defer = final_layer || i + 1 < sub_hi;      // the part's last linear completes X unless the final LN follows
        const bf16_t* sh = (const bf16_t*)a->shift + (int64_t)sb->site * a->shift_site_stride;
        const bf16_t* sc = (const bf16_t*)a->scale + (int64_t)sb->site * a->scale_site_stride;
        const bf16_t* gt = (const bf16_t*)a->gate + (int64_t)sb->site * a->gate_site_stride;
        if (sb->kind == DRN_SUB_CA) {
            if (f.pending) {
                // two cross-attention blocks in a row (not in FA-CA-MLP): X must be complete before the stand-alone add
                if (f.deferred) {
                    DRN_TRY(drn_splitk_gate_res_ln_modulate(a->gemm_ws, f.deferred, a->X, f.deferred_gate, nullptr, sh, sc, a->H, M, D,
                                                            a->S, a->eps, stream));       // (H is scratch here)
                    f.deferred = 0;
                }
                DRN_TRY(drn_bcast_add(a->X, f.pending, M, D, a->S, stream));
            }
            f.pending = (const bf16_t*)a->addvec + (int64_t)sb->ca_index * a->addvec_stride;
            continue;
        }
        DRN_TRY(f.ln_next(sh, sc, mxf));
        if (sb->kind == DRN_SUB_FA) {
            DRN_TRY(f.linear({.a = a->H, .a_mx = h_mx, .w = sb->w_a, .sw = sb->s_a, .c = a->QKV, .M = M, .N = 3 * D, .K = D,
                              .epi = DRN_EPI_NONE}));
            // the 32x32x16 body has no MX epilogue: that site keeps bf16 O + the quantise launch (the same bytes)
            const bool mx_ops = a->attn_precision == 1 && drn_attention_mxfp8_choice(a->heads, a->S) == 1;      // from ONE clip's tokens
            const bool o_mx = mxf && (mx_ops || drn_attention_mx_available());
            DRN_TRY(f.self_attention(sb, mx_ops, o_mx));
            DRN_TRY(f.linear({.a = a->O, .a_mx = o_mx ? act : none, .w = sb->w_b, .sw = sb->s_b, .c = a->X, .M = M, .N = D, .K = D,
                              .epi = DRN_EPI_GATE_RES, .gate = gt, .residual = a->X, .may_defer = may_defer}));
        } else {
            // mx_fused: MLP-up reads AQ | AS and writes U as MX into UQ | US (a second buffer: written while AQ is read) where the
            // GELU -> MX epilogue exists; a sliced MLP-up writes bf16 U and MLP-down quantises it by launch
            bool u_mx = false;
            DRN_TRY(f.linear({.a = a->H, .a_mx = h_mx, .w = sb->w_a, .sw = sb->s_a, .c = a->U, .c_mx = mxf ? uact : none, .M = M,
                              .N = a->hidden, .K = D, .epi = DRN_EPI_GELU}, &u_mx));
            DRN_TRY(f.linear({.a = a->U, .a_mx = u_mx ? uact : none, .w = sb->w_b, .sw = sb->s_b, .c = a->X, .M = M, .N = D,
                              .K = a->hidden, .epi = DRN_EPI_GATE_RES, .gate = gt, .residual = a->X, .may_defer = may_defer}));
        }
    }
    // final layer (CleanGeneralDIT.py:583-590): LN + modulate with the first 2D of the LoRA vector, Linear(D -> n_final)
    if (!final_layer) return DRN_OK;
    DRN_TRY(f.ln_next((const bf16_t*)a->final_shift, (const bf16_t*)a->final_scale, false));
    return f.linear_bf16({.a = a->H, .w = a->w_final, .c = a->Y, .M = M, .N = a->n_final, .K = D, .epi = DRN_EPI_NONE});
}

extern "C" int drn_dit_forward(const drn_dit_forward_args* a, void* stream) {
    if (!a) return DRN_EINVAL;
    return drn_dit_forward_range(a, 0, a->n_sub, DRN_DIT_EMBED | DRN_DIT_FINAL, stream);
}
