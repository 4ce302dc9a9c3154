"""Whole-DiT parity on the GPU: HipDiT (C ABI kernels) against the reference's golden vectors.

Bound: the reference's own bf16 evaluation drifts from exact arithmetic by e_ref; the HIP
path, which keeps the reference's rounding points but accumulates in a different order, must stay within
1.5 x e_ref of the same fp32 evaluation (bf16-quantised host tables), and within 2 x e_ref of the reference's
bf16 output itself.
"""
import json

import pytest
import torch

from conftest import load_golden, rel_l2, tiny_net

pytestmark = pytest.mark.gpu

CASES = [
    ("dit_tinyA.safetensors", "tinyA", 256, 1, 2, False),
    ("dit_tinyB.safetensors", "tinyB", 512, 2, 4, False),
    ("dit_tinyF_forward.safetensors", "tinyF", 256, 1, 2, True),
    ("dit_wide1.safetensors", "wide1", 4096, 1, 32, False),
]


def _run(pkg, gpu, fixture, tag, D, L, heads, forward):
    gold, meta = load_golden(fixture)
    net = tiny_net(pkg, D, L, heads, forward)
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16, device=gpu)
    F_, h, w = json.loads(meta["latent"])
    x = sw.synth_tensor(tag + ".x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor(tag + ".cond", (1, net["additional_concat_ch"], F_, h, w), torch.float32,
                           scale=1.0).to(torch.bfloat16)
    dit = pkg.dit_engine.HipDiT(net, sd, device=gpu)
    dit.trace = {}
    y = dit(x.to(gpu), torch.tensor(float(meta["sigma"])), cond.to(gpu),
            torch.full((1, 1), int(meta["context_index"]), dtype=torch.long))
    torch.cuda.synchronize()
    return gold, y.cpu(), {k: v.cpu() for k, v in dit.trace.items()}


def test_synthetic_weights_identical_on_device(pkg, gpu):
    net = tiny_net(pkg, 256, 1, 2)
    a = pkg.synthetic_weights.synth_state_dict(net, torch.bfloat16, device="cpu")
    b = pkg.synthetic_weights.synth_state_dict(net, torch.bfloat16, device=gpu)
    for k in a:
        assert torch.equal(a[k], b[k].cpu()), k


@pytest.mark.parametrize("fixture,tag,D,L,heads,forward", CASES)
def test_dit_forward_matches_reference_golden(pkg, gpu, fixture, tag, D, L, heads, forward):
    gold, y, trace = _run(pkg, gpu, fixture, tag, D, L, heads, forward)
    ref16 = gold["out.bf16"]
    exact = gold["out.fp32_tables_bf16"]
    e_ref = rel_l2(ref16, exact)
    e_hip = rel_l2(y, exact)
    d = rel_l2(y, ref16)
    print(f"{tag}: e_ref={e_ref:.3e} e_hip={e_hip:.3e} hip-vs-ref16={d:.3e}")
    # per-sub-block activations localise a failure
    for k in sorted(trace):
        gk = f"{k}.bf16"
        if gk in gold:
            dk = rel_l2(trace[k], gold[gk])
            assert dk < max(4 * e_ref, 2e-2), f"{tag} {k}: rel-L2 {dk:.3e}"
    assert e_hip <= max(1.5 * e_ref, 1e-3), (e_hip, e_ref)
    assert d <= max(2.0 * e_ref, 2e-3), (d, e_ref)


@pytest.mark.parametrize("fixture,tag", [("dit_full28_cfg1.safetensors", "full28"), ("dit_full28_s1024.safetensors", "full28_s1024"),
                                         ("dit_full28_s2048.safetensors", "full28_s2048")])
def test_dit_full_28_blocks_matches_reference(pkg, gpu, full28_dit, fixture, tag):
    """The 7.2 B-parameter model against the reference's own output at BASELINE config 1 (1 x 256 x 256 -> S = 256 tokens,
    split-K weight-streaming GEMMs) and config 2 (512 x 512: 8 frames -> latent (1,64,64), S = 1024; 9 frames -> (2,64,64),
    S = 2048: the 128^2 / 256^2 tile kernels and the split-KV attention plan)."""
    gold, meta = load_golden(fixture)
    sw = pkg.synthetic_weights
    F_, h, w = json.loads(meta["latent"])
    x = sw.synth_tensor(tag + ".x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor(tag + ".cond", (1, 16, F_, h, w), torch.float32, scale=1.0).to(torch.bfloat16)
    y = full28_dit(x.to(gpu), torch.tensor(float(meta["sigma"])), cond.to(gpu),
                   torch.full((1, 1), int(meta["context_index"]), dtype=torch.long)).cpu()
    exact = gold["out.fp32_tables_bf16"]
    e_ref, e_hip, d = rel_l2(gold["out.bf16"], exact), rel_l2(y, exact), rel_l2(y, gold["out.bf16"])
    print(f"{tag}: e_ref={e_ref:.3e} e_hip={e_hip:.3e} hip-vs-ref16={d:.3e}")
    assert e_hip <= max(1.5 * e_ref, 1e-3), (e_hip, e_ref)
    assert d <= max(2.0 * e_ref, 2e-3), (d, e_ref)


def test_batched_forward_equals_per_clip_forwards(pkg, gpu):
    """B clips stacked along the token rows (G-buffer passes / CFG halves): every op is row-local except
    self-attention, which is per clip, so clip b of the batch must reproduce its own B = 1 forward."""
    net = tiny_net(pkg, 512, 2, 4)
    sw = pkg.synthetic_weights
    dit = pkg.dit_engine.HipDiT(net, sw.synth_state_dict(net, torch.bfloat16, device=gpu), device=gpu)
    B, F_, h, w = 3, 2, 16, 16
    x = sw.synth_tensor("bat.x", (B, 16, F_, h, w), torch.float32, scale=2.0).to(torch.bfloat16).to(gpu)
    cond = sw.synth_tensor("bat.c", (B, net["additional_concat_ch"], F_, h, w), torch.float32, scale=1.0).to(torch.bfloat16).to(gpu)
    cis = [0, 3, 4]
    yb = dit(x, torch.tensor(1.25), cond, torch.tensor(cis).view(B, 1))
    assert yb.shape == (B, 16, F_, h, w)
    for b in range(B):
        y1 = dit(x[b:b + 1], torch.tensor(1.25), cond[b:b + 1], cis[b])
        # every launch decision that fixes a summation order (tile kernel, tail split, split-K, split-KV) is taken from ONE
        # clip's rows, so a clip's bits do not depend on what it is batched with
        assert torch.equal(yb[b:b + 1], y1), f"clip {b}: rel-L2 {rel_l2(yb[b:b + 1].cpu(), y1.cpu()):.3e}"
    # clips differ (different conditions / context rows), and a shared condition broadcasts
    assert rel_l2(yb[0:1].cpu(), yb[1:2].cpu()) > 1e-2
    y_shared = dit(x, torch.tensor(1.25), cond[:1], cis)
    assert torch.equal(y_shared[0:1], yb[0:1])
    with pytest.raises(ValueError):
        dit(x, torch.tensor([1.0, 2.0, 3.0]), cond, cis)          # one sigma per batch
    with pytest.raises(ValueError):
        dit(x, torch.tensor(1.0), cond, [0, 1])                   # one index per clip


def test_full_size_block_cfg3_matches_oracle(pkg, gpu):
    """BASELINE config 3 shapes (latent 8 x 72 x 128 -> S = 18 432 tokens, D = 4096, 32 heads), ONE transformer block: the
    256^2 GEMM, the whole-round attention launch and every elementwise kernel at the sizes the bench runs, against the CPU
    oracle on the same seeded inputs (bf16 oracle = what the reference computes, fp32 oracle = the exact answer)."""
    import time
    from oracle import dit_oracle as O
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    net = tiny_net(pkg, 4096, 1, 32)
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16)
    F_, h, w = 8, 72, 128
    x = sw.synth_tensor("full.x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor("full.c", (1, 16, F_, h, w), torch.float32, scale=1.0).to(torch.bfloat16)
    t, ci = torch.tensor(3.0), torch.full((1, 1), 3, dtype=torch.long)
    dit = pkg.dit_engine.HipDiT(net, {k: v.to(gpu) for k, v in sd.items()}, device=gpu)
    y = dit(x.to(gpu), t, cond.to(gpu), ci).cpu()
    t0 = time.time()
    with torch.no_grad():
        ref16 = O.DitOracle(sd, net, dtype=torch.bfloat16).forward(x, t, cond, ci)
        exact = O.DitOracle(sd, net, dtype=torch.float32, tables_dtype=torch.bfloat16).forward(x, t, cond, ci)
    e_ref, e_hip, d = rel_l2(ref16, exact), rel_l2(y, exact), rel_l2(y, ref16)
    print(f"cfg3 one block: e_ref={e_ref:.3e} e_hip={e_hip:.3e} hip-vs-ref16={d:.3e} (oracle {time.time() - t0:.0f}s)")
    assert e_hip <= max(1.5 * e_ref, 1e-3), (e_hip, e_ref)
    assert d <= max(2.0 * e_ref, 2e-3), (d, e_ref)


def test_full_size_forward_variant_block_cfg5_matches_oracle(pkg, gpu):
    """BASELINE config 5 shapes: the FORWARD renderer's network (in_channels 16 + 136 condition channels + mask = 153 -> patch
    embed K = 612, no context embedding: the cross-attention adds exactly to_out(to_v(0)) = 0) at the full clip (latent
    8 x 72 x 128 -> S = 18 432 tokens, D = 4096, 32 heads), ONE transformer block, against the CPU oracle on the same seeded
    inputs.  The reference cannot run this pass as committed; the oracle evaluates its network code by the intent
    of get_forward_renderer_config, pinned at small size by dit_tinyF_forward.safetensors."""
    import time
    from oracle import dit_oracle as O
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    net = tiny_net(pkg, 4096, 1, 32, forward=True)
    assert net["additional_concat_ch"] == 136 and not net["use_context_embedding"]
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16)
    F_, h, w = 8, 72, 128
    x = sw.synth_tensor("fwd.x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor("fwd.c", (1, 136, F_, h, w), torch.float32, scale=1.0).to(torch.bfloat16)
    cond[:, 16::17] = 1.0                                      # the mask channels of the 8 encoded maps (ones: map present)
    t, ci = torch.tensor(7.0), torch.zeros((1, 1), dtype=torch.long)
    dit = pkg.dit_engine.HipDiT(net, {k: v.to(gpu) for k, v in sd.items()}, device=gpu)
    y = dit(x.to(gpu), t, cond.to(gpu), ci).cpu()
    t0 = time.time()
    with torch.no_grad():
        ref16 = O.DitOracle(sd, net, dtype=torch.bfloat16).forward(x, t, cond, ci)
        exact = O.DitOracle(sd, net, dtype=torch.float32, tables_dtype=torch.bfloat16).forward(x, t, cond, ci)
    e_ref, e_hip, d = rel_l2(ref16, exact), rel_l2(y, exact), rel_l2(y, ref16)
    print(f"cfg5 forward-variant block: e_ref={e_ref:.3e} e_hip={e_hip:.3e} hip-vs-ref16={d:.3e} (oracle {time.time() - t0:.0f}s)")
    assert e_hip <= max(1.5 * e_ref, 1e-3), (e_hip, e_ref)
    assert d <= max(2.0 * e_ref, 2e-3), (d, e_ref)


def test_full_model_cfg3_batch_and_determinism(pkg, gpu, full28_dit):
    """The whole 28-block, 7.2 B-parameter model at BASELINE config 3 (S = 18 432 tokens per clip).  No CPU oracle finishes
    this size in test time, so size-independent properties stand in: the forward is deterministic (same bits twice), two
    clips stepped as one batch reproduce their own single-clip forwards BIT FOR BIT (row-local ops, per-clip attention, launch
    plans taken from one clip's rows), and clips with different inputs differ."""
    sw = pkg.synthetic_weights
    dit = full28_dit
    F_, h, w = 8, 72, 128
    x = sw.synth_tensor("f28.x", (2, 16, F_, h, w), torch.float32, device=gpu, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor("f28.c", (2, 16, F_, h, w), torch.float32, device=gpu, scale=1.0).to(torch.bfloat16)
    t = torch.tensor(3.0)
    y0 = dit(x[:1], t, cond[:1], 3)
    y0b = dit(x[:1], t, cond[:1], 3)
    assert torch.equal(y0, y0b)
    y1 = dit(x[1:], t, cond[1:], 1)
    yb = dit(x, t, cond, [3, 1])
    assert torch.isfinite(yb.float()).all()
    e0, e1 = rel_l2(yb[:1].cpu(), y0.cpu()), rel_l2(yb[1:].cpu(), y1.cpu())
    print(f"cfg3 full model: batched vs single rel-L2 {e0:.2e} / {e1:.2e}; clip 0 vs clip 1 {rel_l2(y0.cpu(), y1.cpu()):.2e}")
    assert torch.equal(yb[:1], y0) and torch.equal(yb[1:], y1)
    assert rel_l2(y0.cpu(), y1.cpu()) > 0.1


@pytest.mark.parametrize("D,L,heads,lat,B", [(256, 2, 2, (2, 16, 16), 1), (256, 2, 2, (2, 16, 16), 3), (512, 1, 4, (1, 32, 32), 2),
                                               (1024, 1, 8, (2, 64, 64), 1), (2048, 2, 16, (1, 32, 32), 1), (2048, 1, 16, (1, 32, 32), 3)])
def test_forward_sequencer_equals_per_launch_path(pkg, gpu, D, L, heads, lat, B):
    """drn_dit_forward (ONE C call enqueues patch embed, every sub-block and the final layer; the default on one GPU) against the
    per-launch host path (one ctypes call per kernel; what the traces of the golden tests above and the sharded engine run):
    same kernels, same arguments, same order -> the same bits.  S = 128 / 256 (split-K GEMMs + workspaces) and 2048; at D = 2048
    the sequencer folds the split-K sum + gated residual of the out-projection / MLP-down into the next LayerNorm pass
    (drn_splitk_gate_res_ln_modulate) where the per-launch path runs epilogue kernel and LayerNorm one after the other."""
    net = tiny_net(pkg, D, L, heads)
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16, device=gpu)
    x = sw.synth_tensor("seq.x", (B, 16) + lat, torch.float32, device=gpu, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor("seq.c", (B, 16) + lat, torch.float32, device=gpu, scale=1.0).to(torch.bfloat16)
    ci = [3, 0, 4][:B]
    seq = pkg.dit_engine.HipDiT(net, sd, device=gpu)
    per = pkg.dit_engine.HipDiT(net, sd, device=gpu)
    per._per_launch = True
    assert not seq._per_launch
    # several sigmas prepared at once: the AdaLN table of one sigma is then a strided view (site stride = n_sigmas x 3D)
    for eng in (seq, per):
        eng.prepare_timesteps([80.0, 1.7, 0.02])
    for sigma in (1.7, 80.0):
        y_seq = seq(x, torch.tensor(sigma), cond, ci)
        y_per = per(x, torch.tensor(sigma), cond, ci)
        torch.cuda.synchronize()
        assert torch.isfinite(y_seq.float()).all()
        assert torch.equal(y_seq, y_per), f"sigma {sigma}: max |diff| {(y_seq.float() - y_per.float()).abs().max().item()}"


def test_two_launch_attention_plan_sequencer_equals_per_launch(pkg, gpu, monkeypatch):
    """The smallest clip whose self-attention plan is TWO launches: latent (5, 104, 128) -> 5 x 52 x 64 = 16 640 tokens, 4 heads:
    64 whole q-blocks x 4 heads fill one round of the 256 CUs unsplit, the one q-block left runs as a second launch from query
    16 384 with its keys in 8 chunks + the combine pass.  Every other model-level fixture plans a single launch, so only here do
    the sequencer's walk and the host wrapper's advance q / O / the MX rows by a non-zero first query.  For the four pairs of
    (linear, attention) precision, and the MXFP8 linears also with DRN_MX_FUSED=0 (bf16 attention writing MX from the unsplit
    launch and from the combine pass against bf16 O + quantise launches): sequencer == per-launch at B = 1 and B = 2, clip b of
    the batch == that clip alone, a repeated call == itself.  16 640 >= 2048 tokens: drn_attention_mxfp8_choice is 1 unforced."""
    Nn = pkg.native
    heads, lat, S = 4, (5, 104, 128), 16640
    plan = Nn.attention_plan(1, heads, S, S)
    assert len(plan) == 2 and plan[1][2] > 1, plan
    assert plan == [(0, 16384, 1), (16384, 16640, 8)] and Nn.attention_mxfp8_force(-1) == 0 and Nn.attention_mxfp8_choice(heads, S)
    net = tiny_net(pkg, 512, 2, heads)
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16, device=gpu)
    x = sw.synth_tensor("two.x", (2, 16) + lat, torch.float32, device=gpu, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor("two.c", (2, net["additional_concat_ch"]) + lat, torch.float32, device=gpu, scale=1.0).to(torch.bfloat16)
    t = torch.tensor(1.5)
    H = pkg.dit_engine.HipDiT
    for lin, att, fused in [("bf16", "bf16", "1"), ("mxfp8", "bf16", "1"), ("mxfp8", "bf16", "0"), ("bf16", "mxfp8", "1"),
                            ("mxfp8", "mxfp8", "1")]:
        what = f"linears={lin} attention={att} DRN_MX_FUSED={fused}"
        monkeypatch.setenv("DRN_MX_FUSED", fused)
        monkeypatch.setenv("DRN_PER_LAUNCH", "0")
        seq = H(net, sd, device=gpu, precision=lin, attention_precision=att)
        monkeypatch.setenv("DRN_PER_LAUNCH", "1")
        per = H(net, sd, device=gpu, precision=lin, attention_precision=att)
        monkeypatch.delenv("DRN_PER_LAUNCH")
        monkeypatch.delenv("DRN_MX_FUSED")
        assert per._per_launch and not seq._per_launch and seq._mx_fused == (lin == "mxfp8" and fused == "1"), what
        y1 = seq(x[:1], t, cond[:1], 2)
        assert torch.isfinite(y1.float()).all(), what
        assert torch.equal(y1, seq(x[:1], t, cond[:1], 2)), what + ": run to run"
        assert torch.equal(y1, per(x[:1], t, cond[:1], 2)), what + ": sequencer vs per-launch, B = 1"
        y2 = seq(x, t, cond, [2, 4])
        assert torch.equal(y2, per(x, t, cond, [2, 4])), what + ": sequencer vs per-launch, B = 2"
        assert torch.equal(y2[0:1], y1), what + ": clip 0 of the batch vs alone"
        assert torch.equal(y2[1:2], seq(x[1:2], t, cond[1:2], 4)), what + ": clip 1 of the batch vs alone"
        if (lin, att) == ("mxfp8", "bf16"):                  # fused producers write the bytes the quantise launches write
            y_fused = y1 if fused == "1" else y_fused
            assert torch.equal(y1, y_fused), what + ": fused vs quantise launches"
        del seq, per


def test_forward_sequencer_matches_reference_golden(pkg, gpu):
    """The golden of the two-block tiny model through the sequencer path (no trace): same bound as the per-launch path."""
    fixture, tag, D, L, heads, forward = CASES[1]
    gold, meta = load_golden(fixture)
    net = tiny_net(pkg, D, L, heads, forward)
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16, device=gpu)
    F_, h, w = json.loads(meta["latent"])
    x = sw.synth_tensor(tag + ".x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor(tag + ".cond", (1, net["additional_concat_ch"], F_, h, w), torch.float32, scale=1.0).to(torch.bfloat16)
    dit = pkg.dit_engine.HipDiT(net, sd, device=gpu)
    assert dit.trace is None and not dit._per_launch
    y = dit(x.to(gpu), torch.tensor(float(meta["sigma"])), cond.to(gpu), torch.full((1, 1), int(meta["context_index"]), dtype=torch.long)).cpu()
    e_ref, e_hip = rel_l2(gold["out.bf16"], gold["out.fp32_tables_bf16"]), rel_l2(y, gold["out.fp32_tables_bf16"])
    print(f"{tag} (sequencer): e_ref={e_ref:.3e} e_hip={e_hip:.3e}")
    assert e_hip <= 1.5 * e_ref + 1e-3


def test_kernel_timer_sees_sequencer_launches(pkg, gpu):
    """bench.py's roofline leg: with a KernelTimer set, drn_dit_forward brackets every n-th GEMM / attention call with HIP events."""
    net = tiny_net(pkg, 256, 2, 2)
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16, device=gpu)
    x = sw.synth_tensor("tm.x", (1, 16, 2, 16, 16), torch.float32, device=gpu, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor("tm.c", (1, 16, 2, 16, 16), torch.float32, device=gpu).to(torch.bfloat16)
    dit = pkg.dit_engine.HipDiT(net, sd, device=gpu)
    dit(x, torch.tensor(2.0), cond, 1)
    timer = pkg.native.KernelTimer(sample_every=3)
    pkg.native.set_timer(timer)
    try:
        dit(x, torch.tensor(2.0), cond, 1)
    finally:
        pkg.native.set_timer(None)
    torch.cuda.synchronize()
    summ = timer.summary()
    # per forward: patch embed + 2 x (qkv, out, mlp1, mlp2) + final = 10 GEMM calls, 2 attention calls
    assert summ["gemm"]["launches_seen"] == 10 and summ["gemm"]["launches"] == 4 and summ["gemm"]["ms_total"] > 0
    assert summ["attention"]["launches_seen"] == 2 and summ["attention"]["launches"] == 1 and summ["attention"]["flops"] > 0
