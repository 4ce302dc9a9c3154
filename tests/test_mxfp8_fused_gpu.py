"""MXFP8 producers that write their result quantised, on the GPU.  Every check is torch.equal against the EXISTING unfused kernel
followed by native.mx_quant (the one rule of include/drn.h: no tolerance anywhere): LayerNorm + modulate in every form, the
attention epilogue (unsplit, split keys, the two-launch plan, a batch), the GELU epilogue of both MXFP8 GEMM kernels, and the
engine - fused against DRN_MX_FUSED=0, sequencer against per-launch, the quantise-launch counter, the per-site fall-backs.
Inputs and the branch-coverage assertion come from tests/test_mxfp8_fused_cpu.py, which shows that they expose the plausible
mistakes."""
import json

import pytest
import torch

from conftest import load_golden, rel_l2, tiny_net
from test_mxfp8_fused_cpu import assert_covers, attn_inputs, gelu_inputs, ln_inputs

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def st():
    return torch.cuda.current_stream().cuda_stream


def same_mx(a, b):
    return torch.equal(a.q.view(torch.uint8), b.q.view(torch.uint8)) and torch.equal(a.scales, b.scales)


def assert_same_mx(got, ref, what):
    q, r = got.q.view(torch.uint8), ref.q.view(torch.uint8)
    if not torch.equal(got.scales, ref.scales):
        bad = (got.scales != ref.scales).nonzero()
        pytest.fail(f"{what}: {bad.shape[0]} of {ref.scales.numel()} scale bytes differ; first (row, block): {bad[:6].tolist()}")
    if not torch.equal(q, r):
        bad = (q != r).nonzero()
        pytest.fail(f"{what}: {bad.shape[0]} of {r.numel()} element bytes differ; first (row, col): {bad[:6].tolist()}")


@pytest.fixture()
def hooks(pkg):
    """Default kernel choices whatever an earlier test or the environment left; restored after."""
    lib = pkg.native.load_library()
    small = lib.drn_gemm_mxfp8_force_small_m(1)
    shape = lib.drn_gemm_mxfp8_tall_force_shape(-1)
    lib.drn_ln_force_kernel(-1)
    lib.drn_attention_force_shape16(1)
    yield lib
    lib.drn_gemm_mxfp8_force_small_m(small)
    lib.drn_gemm_mxfp8_tall_force_shape(shape)
    lib.drn_ln_force_kernel(-1)
    lib.drn_attention_force_shape16(-1)


# ------------------------------------------------------------------------------------------------ 4. LayerNorm + modulate
@pytest.mark.parametrize("force", [0, 1])
@pytest.mark.parametrize("rows", [128, 256, 300])
@pytest.mark.parametrize("D", [512, 1024, 4096])
def test_ln_modulate_mx_equals_ln_then_quant(pkg, gpu, hooks, D, rows, force):
    """One wave / four waves per row (D <= 1024 has only the first), with and without the broadcast pre-add, two clips with
    their own shift / scale rows, h = NULL and h given: (hq, hs) == mx_quant(h of drn_ln_modulate), x written back equal."""
    Nn = pkg.native
    hooks.drn_ln_force_kernel(force)
    x0, add, shift, scale = (t.to(gpu) for t in ln_inputs(rows, D, 2, seed=D + rows))
    rpb = rows // 2
    for addv in (None, add):
        xr = x0.clone()
        h_ref = Nn.ln_modulate(xr, shift, scale, add_vec=addv, rows_per_batch=rpb)
        ref = Nn.mx_quant(h_ref)
        if addv is not None:
            assert_covers(h_ref.cpu(), f"ln D={D} rows={rows}")
        for with_h in (False, True):
            x = x0.clone()
            h = torch.full_like(x, 7.0) if with_h else None
            got = Nn.ln_modulate(x, shift, scale, out=h, add_vec=addv, rows_per_batch=rpb, out_mx=True)
            assert_same_mx(got, ref, f"ln D={D} rows={rows} force={force} add={addv is not None} h={with_h}")
            assert torch.equal(x, xr)
            if with_h:
                assert torch.equal(h, h_ref)


@pytest.mark.parametrize("splits", [2, 4])
@pytest.mark.parametrize("rows", [128, 256, 300])
def test_splitk_fold_mx_equals_fold_then_quant(pkg, gpu, hooks, rows, splits):
    """drn_splitk_gate_res_ln_modulate_mx against drn_splitk_gate_res_ln_modulate + mx_quant (D = 4096: the fold needs D > 1024)."""
    Nn, lib, D = pkg.native, hooks, 4096
    x0, add, shift, scale = (t.to(gpu) for t in ln_inputs(rows, D, 2, seed=7 * rows + splits))
    g = torch.Generator(device="cpu").manual_seed(rows + splits)
    part = (torch.randn((splits, rows, D), generator=g) * 0.7).to(gpu)
    gate = (torch.randn((2, D), generator=g) * 0.5).to(BF).to(gpu)
    rpb = rows // 2
    for addv in (None, add):
        ap = addv.data_ptr() if addv is not None else None
        xr, h_ref = x0.clone(), torch.empty_like(x0)
        assert lib.drn_splitk_gate_res_ln_modulate(part.data_ptr(), splits, xr.data_ptr(), gate.data_ptr(), ap, shift.data_ptr(),
                                                   scale.data_ptr(), h_ref.data_ptr(), rows, D, rpb, 1e-6, st()) == 0
        ref = Nn.mx_quant(h_ref)
        assert_covers(h_ref.cpu(), f"fold rows={rows}")
        for with_h in (False, True):
            x = x0.clone()
            h = torch.full_like(x, 7.0) if with_h else None
            got = Nn.mx_empty(rows, D, gpu)
            assert lib.drn_splitk_gate_res_ln_modulate_mx(part.data_ptr(), splits, x.data_ptr(), gate.data_ptr(), ap,
                                                          shift.data_ptr(), scale.data_ptr(), h.data_ptr() if with_h else None,
                                                          got.q.data_ptr(), got.scales.data_ptr(), rows, D, rpb, 1e-6, st()) == 0
            assert_same_mx(got, ref, f"fold rows={rows} splits={splits} add={addv is not None} h={with_h}")
            assert torch.equal(x, xr)
            if with_h:
                assert torch.equal(h, h_ref)


# ------------------------------------------------------------------------------------------------ 5. attention
@pytest.mark.parametrize("S", [128, 256, 1024, 2304])
@pytest.mark.parametrize("heads", [4, 32])
def test_attention_mx_equals_attention_then_quant(pkg, gpu, hooks, heads, S):
    """The 16x16x32 body unsplit and with the keys cut in 2 and 4 (the MX epilogue then sits in the combine pass), the plan of
    native.attention_plan (two launches over one output buffer where it has two), a batch of 2, o = NULL and o given."""
    Nn = pkg.native
    B = 2
    q, k, v = (t.to(gpu) for t in attn_inputs(B, S, heads, seed=heads + S))
    HD = heads * 128
    plans = [1, 2, 4, None]
    if S == 2304 and heads == 32:
        assert len(Nn.attention_plan(1, heads, S, S)) == 2           # whole rounds unsplit + a split tail, one output buffer
    for kv in plans:
        o_ref = Nn.attention(q, k, v, heads=heads, kv_splits=kv)
        ref = Nn.mx_quant(o_ref.view(B * S, HD))
        if kv == 1:
            assert_covers(o_ref.view(B * S, HD).cpu(), f"attention heads={heads} S={S}")
        got = Nn.attention(q, k, v, heads=heads, kv_splits=kv, out_mx=True)
        assert_same_mx(got, ref, f"attention heads={heads} S={S} kv_splits={kv} o=NULL")
        o = torch.full_like(o_ref, 7.0)
        got = Nn.attention(q, k, v, out=o, heads=heads, kv_splits=kv, out_mx=True)
        assert_same_mx(got, ref, f"attention heads={heads} S={S} kv_splits={kv} o given")
        assert torch.equal(o, o_ref)
    # one clip alone gives the rows of the batch (the MX rows of clip b start at b * S)
    got1 = Nn.attention(q[1:2], k[1:2], v[1:2], heads=heads, kv_splits=1, out_mx=True)
    ref2 = Nn.mx_quant(Nn.attention(q, k, v, heads=heads, kv_splits=1).view(B * S, HD))
    assert torch.equal(got1.q.view(torch.uint8), ref2.q.view(torch.uint8)[S:]) and torch.equal(got1.scales, ref2.scales[S:])


def test_attention_mx_strided_qkv_and_32x32_body_refuses(pkg, gpu, hooks):
    """q | k | v as column slices of one [S, 3 D] buffer (what the engine passes); the 32x32x16 body has no MX epilogue: the
    wrapper raises, the C entry returns DRN_EINVAL and writes nothing."""
    Nn, lib = pkg.native, hooks
    heads, S = 4, 256
    HD = heads * 128
    q, k, v = attn_inputs(1, S, heads, seed=3)
    qkv = torch.cat([q, k, v], dim=2).to(gpu)
    qs, ks, vs = qkv[:, :, :HD], qkv[:, :, HD:2 * HD], qkv[:, :, 2 * HD:]
    ref = Nn.mx_quant(Nn.attention(qs, ks, vs, heads=heads).view(S, HD))
    assert_same_mx(Nn.attention(qs, ks, vs, heads=heads, out_mx=True), ref, "strided q|k|v")
    lib.drn_attention_force_shape16(0)
    try:
        with pytest.raises(RuntimeError):
            Nn.attention(qs, ks, vs, heads=heads, out_mx=True)
        mx = Nn.mx_empty(S, HD, gpu)
        mx.q.view(torch.uint8).fill_(0x55)
        mx.scales.fill_(0x55)
        rc = lib.drn_attention_bf16_mx(qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), None, mx.q.data_ptr(), mx.scales.data_ptr(), 1,
                                       heads, S, S, 3 * HD, 3 * HD, 3 * HD, HD, 0, 0, 0, 0, 0.0884, st())
        torch.cuda.synchronize()
        assert rc == -1 and bool((mx.q.view(torch.uint8) == 0x55).all()) and bool((mx.scales == 0x55).all())
        # the documented fall-back: bf16 output of that body + the quantise launch
        o32 = Nn.attention(qs, ks, vs, heads=heads)
        assert torch.isfinite(o32).all()
    finally:
        lib.drn_attention_force_shape16(1)


# ------------------------------------------------------------------------------------------------ 6. GELU epilogue of the MXFP8 GEMMs
def _gelu_case(pkg, gpu, M, N, K, rpb, what):
    Nn = pkg.native
    a, w = gelu_inputs(M, N, K, seed=M + N + K)
    aq, wq = Nn.mx_quant(a.to(gpu)), Nn.mx_quant(w.to(gpu))
    u = Nn.gemm_mxfp8(aq, wq, epilogue=Nn.EPI_GELU, rows_per_batch=rpb)
    ref = Nn.mx_quant(u)
    assert_covers(u.cpu(), what)
    got = Nn.gemm_mxfp8(aq, wq, epilogue=Nn.EPI_GELU, rows_per_batch=rpb, out_mx=True)
    assert_same_mx(got, ref, what)
    reuse = Nn.mx_empty(M, N, gpu)
    assert Nn.gemm_mxfp8(aq, wq, epilogue=Nn.EPI_GELU, rows_per_batch=rpb, out_mx=reuse) is reuse
    assert_same_mx(reuse, ref, what + " (out_mx reused)")


@pytest.mark.parametrize("N,K", [(16384, 4096), (2048, 512)])
@pytest.mark.parametrize("M", [300, 2304])
def test_gemm_gelu_mx_256_tiles(pkg, gpu, hooks, M, N, K):
    """drn_gemm_mxfp8's 256 x 256 kernel (choice 0): a ragged last tile (M = 300: rows masked on store) and whole tiles."""
    assert pkg.native.mx_gemm_plan(M, N, K) == 0
    _gelu_case(pkg, gpu, M, N, K, None, f"gelu 256x256 M={M} N={N} K={K}")


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("N,K", [(16384, 4096), (2048, 512)])
@pytest.mark.parametrize("M,rpb", [(256, None), (512, None), (512, 256)])
def test_gemm_gelu_mx_few_tokens(pkg, gpu, hooks, M, rpb, N, K, shape):
    """The few-token kernel, unsplit, in both tile shapes; a two-clip stack takes the plan of one clip."""
    hooks.drn_gemm_mxfp8_tall_force_shape(shape)
    assert pkg.native.mx_gemm_plan(M, N, K, rpb) == 1
    _gelu_case(pkg, gpu, M, N, K, rpb, f"gelu few-token shape={shape} M={M} rpb={rpb} N={N} K={K}")


def test_gemm_gelu_mx_sliced_choice_refuses(pkg, gpu, hooks):
    Nn, lib = pkg.native, hooks
    M, N, K = 256, 4096, 16384
    assert Nn.mx_gemm_plan(M, N, K) > 1
    a, w = gelu_inputs(M, N, K, seed=1)
    aq, wq = Nn.mx_quant(a.to(gpu)), Nn.mx_quant(w.to(gpu))
    mx = Nn.mx_empty(M, N, gpu)
    mx.scales.fill_(0x55)
    rc = lib.drn_gemm_mxfp8_gelu_mx(aq.q.data_ptr(), aq.scales.data_ptr(), wq.q.data_ptr(), wq.scales.data_ptr(), mx.q.data_ptr(),
                                    mx.scales.data_ptr(), M, N, K, 0, st())
    torch.cuda.synchronize()
    assert rc == -1 and bool((mx.scales == 0x55).all())
    with pytest.raises(ValueError):
        Nn.gemm_mxfp8(aq, wq, epilogue=Nn.EPI_GELU, out_mx=True)


# ------------------------------------------------------------------------------------------------ 7. engine
def _inputs(pkg, gpu, net, tag, B, latent):
    sw = pkg.synthetic_weights
    F_, h, w = latent
    x = sw.synth_tensor(tag + ".x", (B, 16, F_, h, w), torch.float32, scale=2.0).to(BF).to(gpu)
    cond = sw.synth_tensor(tag + ".c", (B, net["additional_concat_ch"], F_, h, w), torch.float32).to(BF).to(gpu)
    return x, cond


def _engines(pkg, gpu, net, sd, monkeypatch):
    """(sequencer fused, sequencer with the switch off, per-launch fused, per-launch with the switch off)"""
    H = pkg.dit_engine.HipDiT
    out = []
    for per in ("0", "1"):
        for fused in ("1", "0"):
            monkeypatch.setenv("DRN_PER_LAUNCH", per)
            monkeypatch.setenv("DRN_MX_FUSED", fused)
            out.append(H(net, sd, device=gpu, precision="mxfp8"))
    monkeypatch.delenv("DRN_PER_LAUNCH")
    monkeypatch.delenv("DRN_MX_FUSED")
    assert [(e._per_launch, e._mx_fused) for e in out] == [(False, True), (False, False), (True, True), (True, False)]
    assert H(net, sd, device=gpu, precision="mxfp8")._mx_fused and not H(net, sd, device=gpu)._mx_fused       # the defaults
    return out


@pytest.mark.parametrize("tag,D,L,heads,latent", [("tinyB", 512, 2, 4, (2, 16, 16)), ("wide1", 4096, 1, 32, (1, 32, 32))])
def test_engine_fused_equals_unfused(pkg, gpu, hooks, monkeypatch, tag, D, L, heads, latent):
    """tinyB (S = 128: ragged 256-row tiles, every product on drn_gemm_mxfp8) and wide1 (S = 256: the few-token kernels, sliced
    out-proj / MLP-down and the deferred LayerNorm fold): fused == DRN_MX_FUSED=0 on the sequencer and per launch, a two-clip batch
    reproduces each clip alone, and the counter of quantise launches says what ran."""
    Nn = pkg.native
    net = tiny_net(pkg, D, L, heads)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
    S = latent[0] * (latent[1] // 2) * (latent[2] // 2)
    plans = [Nn.mx_gemm_plan(S, n, k) for n, k in [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]]
    if tag == "tinyB":
        assert S == 128 and plans == [0, 0, 0, 0]
    else:
        assert S == 256 and plans[0] == 1 and plans[2] == 1 and plans[1] > 1 and plans[3] > 1
    seq_f, seq_u, per_f, per_u = _engines(pkg, gpu, net, sd, monkeypatch)
    pairs = sum(1 for subs in seq_f.blocks for sb in subs if sb["kind"] == "fa")
    assert pairs == L and sum(1 for subs in seq_f.blocks for sb in subs if sb["kind"] == "mlp") == L
    x, cond = _inputs(pkg, gpu, net, "mxf." + tag, 2, latent)
    t = torch.tensor(1.5)

    def run(engine, *args):
        Nn.mx_quant_calls(reset=True)
        y = engine(*args)
        torch.cuda.synchronize()
        return y, Nn.mx_quant_calls(reset=True)

    y_u, n_u = run(seq_u, x[:1], t, cond[:1], 2)
    assert torch.isfinite(y_u).all() and n_u == 4 * pairs
    y_f, n_f = run(seq_f, x[:1], t, cond[:1], 2)
    assert n_f == 0
    assert torch.equal(y_f, y_u)
    y, n = run(per_f, x[:1], t, cond[:1], 2)
    assert n == 0 and torch.equal(y, y_u)
    y, n = run(per_u, x[:1], t, cond[:1], 2)
    assert n == 4 * pairs and torch.equal(y, y_u)
    assert torch.equal(seq_f(x[:1], t, cond[:1], 2), y_u)                   # run to run
    # two clips stacked: fused == unfused == each clip alone
    y2, n2 = run(seq_f, x, t, cond, [2, 4])
    assert n2 == 0
    assert torch.equal(y2, seq_u(x, t, cond, [2, 4])) and torch.equal(y2, per_f(x, t, cond, [2, 4]))
    assert torch.equal(y2[0:1], y_u) and torch.equal(y2[1:2], seq_f(x[1:2], t, cond[1:2], 4))
    # the 32x32x16 attention body has no MX epilogue: exactly the out-proj sites quantise by launch; compared with the unfused
    # run on the same body (the two bodies sum in different orders)
    hooks.drn_attention_force_shape16(0)
    try:
        y32_u, n = run(seq_u, x[:1], t, cond[:1], 2)
        assert n == 4 * pairs
        y32_f, n = run(seq_f, x[:1], t, cond[:1], 2)
        assert n == pairs and torch.equal(y32_f, y32_u)
        y32_p, n = run(per_f, x[:1], t, cond[:1], 2)
        assert n == pairs and torch.equal(y32_p, y32_u)
    finally:
        hooks.drn_attention_force_shape16(1)
    if tag == "wide1":
        # (a sliced MLP-up: test_engine_sliced_mlp_up_keeps_its_quantise_launch)  With the small-M path off every product runs on the 256 x 256 kernel, still without a quantise launch
        hooks.drn_gemm_mxfp8_force_small_m(0)
        try:
            y0_f, n = run(seq_f, x[:1], t, cond[:1], 2)
            assert n == 0 and torch.equal(y0_f, seq_u(x[:1], t, cond[:1], 2))
        finally:
            hooks.drn_gemm_mxfp8_force_small_m(1)


def test_engine_sliced_mlp_up_keeps_its_quantise_launch(pkg, gpu, hooks, monkeypatch):
    """The per-site fall-back for an MLP-up that is sliced along K: D = 4096 with mlp_ratio 1 (hidden = D) at S = 256 gives MLP-up
    the choice of wide1's out-proj (> 1), so its GELU lives in the reduce launch, U leaves as bf16 and the MLP-down site alone
    quantises by launch - on the sequencer and per launch, one clip and two.  Same bits as DRN_MX_FUSED=0 either way."""
    Nn = pkg.native
    D, L, heads, latent = 4096, 2, 32, (1, 32, 32)
    net = tiny_net(pkg, D, L, heads)
    net["mlp_ratio"] = 1.0
    S = latent[0] * (latent[1] // 2) * (latent[2] // 2)
    assert S == 256 and Nn.mx_gemm_plan(S, D, D) > 1 and Nn.mx_gemm_plan(S, 3 * D, D) == 1
    sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
    seq_f, seq_u, per_f, per_u = _engines(pkg, gpu, net, sd, monkeypatch)
    n_fa = sum(1 for subs in seq_f.blocks for sb in subs if sb["kind"] == "fa")
    n_mlp = sum(1 for subs in seq_f.blocks for sb in subs if sb["kind"] == "mlp")
    assert n_fa == L and n_mlp == L
    x, cond = _inputs(pkg, gpu, net, "mxf.sliced", 2, latent)
    t = torch.tensor(1.5)

    def run(engine, *args):
        Nn.mx_quant_calls(reset=True)
        y = engine(*args)
        torch.cuda.synchronize()
        return y, Nn.mx_quant_calls(reset=True)

    y_u, n = run(seq_u, x[:1], t, cond[:1], 2)
    assert torch.isfinite(y_u).all() and n == 2 * n_fa + 2 * n_mlp
    y, n = run(seq_f, x[:1], t, cond[:1], 2)
    assert n == n_mlp and torch.equal(y, y_u)                   # 0 per FA, 1 per MLP: the MLP-down site
    y, n = run(per_f, x[:1], t, cond[:1], 2)
    assert n == n_mlp and torch.equal(y, y_u)
    y, n = run(per_u, x[:1], t, cond[:1], 2)
    assert n == 2 * n_fa + 2 * n_mlp and torch.equal(y, y_u)
    y2, n = run(seq_f, x, t, cond, [2, 4])
    assert n == n_mlp
    assert torch.equal(y2, seq_u(x, t, cond, [2, 4])) and torch.equal(y2, per_f(x, t, cond, [2, 4]))
    assert torch.equal(y2[0:1], y_u) and torch.equal(y2[1:2], seq_f(x[1:2], t, cond[1:2], 4))
    # an FA-only count: with the 32x32x16 attention body on top, the out-proj sites quantise by launch as well
    hooks.drn_attention_force_shape16(0)
    try:
        y32_u, _ = run(seq_u, x[:1], t, cond[:1], 2)
        y32, n = run(seq_f, x[:1], t, cond[:1], 2)
        assert n == n_fa + n_mlp and torch.equal(y32, y32_u)
    finally:
        hooks.drn_attention_force_shape16(1)


def test_engine_full_28_blocks_fused_equals_unfused(pkg, gpu, hooks):
    """The 28-block model at cfg 1 (dit_full28_cfg1), all four routes on one engine: sequencer and per launch, fused and with the
    switch off.  All equal, so the error against the golden is the identical figure; 0 quantise launches against 4 x 28."""
    Nn = pkg.native
    net = tiny_net(pkg, 4096, 28, 32)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
    dit = pkg.dit_engine.HipDiT(net, sd, device=gpu, precision="mxfp8")
    del sd
    torch.cuda.empty_cache()
    assert dit._mx_fused and not dit._per_launch
    sw = pkg.synthetic_weights
    gold, meta = load_golden("dit_full28_cfg1.safetensors")
    F_, h, w = json.loads(meta["latent"])
    x = sw.synth_tensor("full28.x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(BF).to(gpu)
    cond = sw.synth_tensor("full28.cond", (1, 16, F_, h, w), torch.float32, scale=1.0).to(BF).to(gpu)
    t = torch.tensor(float(meta["sigma"]))
    ci = torch.full((1, 1), int(meta["context_index"]), dtype=torch.long)
    exact = gold["out.fp32_tables_bf16"]
    out = {}
    try:
        # the switches DRN_PER_LAUNCH=1 / DRN_MX_FUSED=0 set at construction, flipped on the one 14.5 GB engine instead of four
        for per in (False, True):
            for fused in (True, False):
                dit._per_launch, dit._mx_fused = per, fused
                Nn.mx_quant_calls(reset=True)
                y = dit(x, t, cond, ci).float().cpu()
                out[(per, fused)] = (y, Nn.mx_quant_calls(reset=True))
    finally:
        dit._per_launch, dit._mx_fused = False, True
    y_u, n_u = out[(False, False)]
    e_u = rel_l2(y_u, exact)
    assert torch.isfinite(y_u).all() and n_u == 4 * 28
    for (per, fused), (y, n) in out.items():
        e = rel_l2(y, exact)
        print(f"full28 cfg1 mxfp8 per_launch={per} fused={fused}: e={e:.6e} quantise launches {n}")
        assert n == (0 if fused else 4 * 28), (per, fused, n)
        assert torch.equal(y, y_u) and e == e_u, (per, fused)
    del dit
    torch.cuda.empty_cache()
