"""MXFP8 self-attention (HipDiT(attention_precision="mxfp8"), include/drn.h, csrc/attention_mx.hip) on the GPU: the two producers bit
for bit against the torch emulation, the kernel's lane maps with exact data, the kernel against the emulation of its arithmetic on
random data, and the model.  References, emulation, grid and bounds come from tests/mx_attn_refs.py; tests/test_mx_attn_refs_cpu.py
proves on the CPU that these bounds pass the correct emulation at every grid case and fail the mutated ones.  Every kernel output
lives in a guard band of tests/dit_refs.py and every launch runs twice (same bits, guards intact)."""
import functools
import json

import pytest
import torch

import dit_refs as D
import mx_attn_refs as R
import mx_emul as MX
from conftest import load_golden, rel_l2, tiny_net

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U8 = torch.uint8
H = R.HEADS
HD = H * 128


def _bits(t):
    return t.contiguous().view(U8).cpu()


def _guard_u8(t, dev):
    """A uint8 / e4m3 tensor inside a guard band on the device: -> (buffer, view of t's shape, uint8)."""
    n = t.numel()
    buf, view = D.guarded(1, n, n, 1, dev, dtype=U8)
    view.copy_(t.contiguous().view(U8).reshape(1, n))
    return buf, view.view(t.shape)


@functools.lru_cache(maxsize=None)
def _policy(pkg):
    return pkg.native.attention_mxfp8_params()


def _launch(pkg, dev, ops, B, Sq, Sk, ns, mx_out=False):
    """The kernel on the operands of `ops`, twice, outputs in guard bands: -> bf16 [B, Sq, HD] on the CPU (mx_out: plus the MX
    output bytes (q, scales) written beside it)."""
    Nn = pkg.native
    f8 = torch.float8_e4m3fn
    keep = []
    dv = {}
    for name in ("qq", "qs", "kq", "ks", "vt", "vs"):
        buf, view = _guard_u8(ops[name], dev)
        keep.append((buf, view))
        dv[name] = view
    qm = Nn.MxTensor(dv["qq"].view(f8), dv["qs"])
    km = Nn.MxTensor(dv["kq"].view(f8), dv["ks"])
    vt, vs = dv["vt"].view(f8), dv["vs"]
    outs = []
    for rep in range(2):
        if mx_out:
            obuf, o = D.guarded(B * Sq, HD, HD, 2, dev)
            qbuf, oq = D.guarded(B * Sq, HD, HD, 2, dev, dtype=U8)
            sbuf, osc = D.guarded(B * Sq, HD // 32, HD // 32, 8, dev, dtype=U8)
            mx = Nn.MxTensor(oq.view(f8), osc)
            Nn.attention_mxfp8(qm, km, vt, vs, B, Sq, Sk, out=o.view(B, Sq, HD), out_mx=mx, kv_splits=ns)
            torch.cuda.synchronize()
            for b_, v_ in ((obuf, o), (qbuf, oq), (sbuf, osc)):
                D.assert_guard_intact(b_, v_)
            outs.append((o.view(B, Sq, HD).cpu(), oq.cpu(), osc.cpu()))
        else:
            obuf, o = D.guarded(Sq, HD, HD + 64, 2, dev, batches=B, batch_gap=128)
            o3 = o if B > 1 else o.unsqueeze(0)
            Nn.attention_mxfp8(qm, km, vt, vs, B, Sq, Sk, out=o3, kv_splits=ns)
            torch.cuda.synchronize()
            D.assert_guard_intact(obuf, o)
            outs.append((o3.cpu(),))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b)), "two launches on the same operands differ"
    for buf, view in keep:                                  # the operands were only read
        D.assert_guard_intact(buf, view.reshape(1, -1))
    assert not D.is_sentinel(outs[0][0]).any(), "an output element was not written"
    return outs[0] if mx_out else outs[0][0]


# ------------------------------------------------------------------------------------------------ 1. producers, bit for bit
@pytest.mark.parametrize("write_bf16", [0, 1])
@pytest.mark.parametrize("which", ["qk", "q", "k"])
def test_qk_norm_rope_mx_equals_twin_then_quantize(pkg, gpu, write_bf16, which):
    """300 tokens = two clips of 150, q and k slices of a [tokens, 3D] buffer (ldq = 3D), table rows from pos_offset 5."""
    Nn = pkg.native
    tokens, tpb, off = 300, 150, 5
    base = D.rnd((tokens, 3 * HD), 1.5, seed=21)
    wq, wk = D.rnd((128,), 1.0, seed=22), D.rnd((128,), 1.0, seed=23)
    g = torch.Generator(device="cpu").manual_seed(24)
    ang = torch.rand((tpb + off, 128), generator=g) * 6.28
    cos, sin = ang.cos().to(BF), ang.sin().to(BF)
    dq, dk = which in ("qk", "q"), which in ("qk", "k")
    ref = base.to(gpu)
    Nn.qk_norm_rope(ref[:, :HD] if dq else None, ref[:, HD:2 * HD] if dk else None, wq.to(gpu) if dq else None,
                    wk.to(gpu) if dk else None, cos.to(gpu), sin.to(gpu), H, tokens_per_batch=tpb, pos_offset=off)
    torch.cuda.synchronize()
    ref = ref.cpu()
    want = {n: MX.quantize(ref[:, c0:c0 + HD].contiguous()) for n, c0, on in (("q", 0, dq), ("k", HD, dk)) if on}
    got = []
    for rep in range(2):
        xbuf, x = D.guarded(tokens, 3 * HD, 3 * HD, 2, gpu)
        x.copy_(base)
        outs = {}
        for n in want:
            eb, e = D.guarded(tokens, HD, HD, 2, gpu, dtype=U8)
            sb, s = D.guarded(tokens, HD // 32, HD // 32, 8, gpu, dtype=U8)
            outs[n] = (eb, e, sb, s)
        mk = lambda n: Nn.MxTensor(outs[n][1].view(torch.float8_e4m3fn), outs[n][3]) if n in outs else None
        Nn.qk_norm_rope_mx(x[:, :HD] if dq else None, x[:, HD:2 * HD] if dk else None, wq.to(gpu) if dq else None,
                           wk.to(gpu) if dk else None, cos.to(gpu), sin.to(gpu), H, tokens_per_batch=tpb, pos_offset=off,
                           write_bf16=bool(write_bf16), out_q=mk("q"), out_k=mk("k"))
        torch.cuda.synchronize()
        D.assert_guard_intact(xbuf, x)
        for n, (eb, e, sb, s) in outs.items():
            D.assert_guard_intact(eb, e)
            D.assert_guard_intact(sb, s)
            assert torch.equal(s.cpu(), want[n][1]), (n, "scales")
            assert torch.equal(e.cpu(), _bits(want[n][0])), (n, f"{(e.cpu() != _bits(want[n][0])).sum().item()} element bytes differ")
        # the bf16 buffer: the twin's result where write_bf16, the input elsewhere (v and an absent q / k are never touched)
        expect = ref if write_bf16 else base
        assert torch.equal(_bits(x.cpu()), _bits(expect))
        got.append({n: (o[1].cpu(), o[3].cpu()) for n, o in outs.items()})
    assert all(torch.equal(got[0][n][i], got[1][n][i]) for n in got[0] for i in (0, 1))


@pytest.mark.parametrize("Sk", [128, 200, 288])
def test_mx_quant_vt_bit_exact(pkg, gpu, Sk):
    """B = 2, v as the last third of a [B, Sk, 3D] buffer; the padded tail is zero with scale byte 0."""
    Nn = pkg.native
    B = 2
    base = D.rnd((B, Sk, 3 * HD), 2.0, seed=30 + Sk)
    base[0, : min(Sk, 40), 2 * HD + 3] = 0.0                         # an all-zero 32-key block of one (head, d)
    base[1, 5, 2 * HD + 7] = 300.0                                  # an outlier
    want_t, want_s = R.quantize_vt(base[:, :, 2 * HD:].contiguous(), H)
    Skp = R.pad128(Sk)
    res = []
    for rep in range(2):
        xbuf, x = D.guarded(Sk, 3 * HD, 3 * HD, 2, gpu, batches=B, batch_gap=64)
        x.copy_(base)
        tb, t = D.guarded(1, B * HD * Skp, B * HD * Skp, 1, gpu, dtype=U8)
        sb, s = D.guarded(1, B * HD * Skp // 32, B * HD * Skp // 32, 1, gpu, dtype=U8)
        Nn.mx_quant_vt(x[:, :, 2 * HD:], H, out=(t.view(torch.float8_e4m3fn).view(B, H, 128, Skp), s.view(B, H, 128, Skp // 32)))
        torch.cuda.synchronize()
        for b_, v_ in ((xbuf, x), (tb, t), (sb, s)):
            D.assert_guard_intact(b_, v_)
        res.append((t.cpu().view(B, H, 128, Skp), s.cpu().view(B, H, 128, Skp // 32)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    t, s = res[0]
    assert torch.equal(s, want_s), "scales"
    assert torch.equal(t, _bits(want_t).view(B, H, 128, Skp)), f"{(t != _bits(want_t).view(B, H, 128, Skp)).sum().item()} element bytes differ"
    if Skp > Sk:
        assert int(t[..., Sk:].max()) == 0, "the padded keys must be zero bytes"
    assert int(s[0, 0, 3, 0]) == 0                                  # the all-zero block: scale byte 0


# ------------------------------------------------------------------------------------------------ 2. lane maps with exact data
@pytest.mark.parametrize("ns", [1, 2, 3])
def test_uniform_scores_exact_sum(pkg, gpu, ns):
    ops, ref = R.uniform_case()
    out = _launch(pkg, gpu, ops, 1, 300, 200, ns)
    d = (out.double() - ref).abs()
    ulp = torch.maximum(ref.abs(), out.double().abs()) * 2.0 ** -7
    worst = (d / ulp.clamp_min(1e-30)).max().item()
    print(f"uniform ns={ns}: worst {worst:.3f} bf16 ulp of sum / Sk")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("ns", [1, 2, 3])
def test_spike_one_hot_rows(pkg, gpu, ns):
    ops, pi, want = R.spike_case()
    out = _launch(pkg, gpu, ops, 1, 300, 384, ns)
    if not torch.equal(out, want):
        bad = (out != want).any(-1).nonzero().flatten()
        pytest.fail(f"{bad.numel()} of 300 rows differ from their V row; first queries {bad[:8].tolist()} -> keys {pi[bad[:8]].tolist()}")


# ------------------------------------------------------------------------------------------------ 3. random data
@functools.lru_cache(maxsize=None)
def _case(c, policy):
    ops = R.random_case(c)
    emul = R.attention_emul(ops["qq"], ops["qs"], ops["kq"], ops["ks"], ops["vt"], ops["vs"], c.B, c.Sq, c.Sk, policy, ns=c.ns)
    return ops, rel_l2(emul.float(), ops["exact"])


@pytest.mark.parametrize("c", R.GRID, ids=R.case_id)
def test_random_against_emulation(pkg, gpu, c):
    ops, e_emul = _case(c, _policy(pkg))
    out = _launch(pkg, gpu, ops, c.B, c.Sq, c.Sk, c.ns)
    ok, e_hip, worst = R.check_bounds(out, ops, e_emul)
    print(f"mx attention {R.case_id(c)}: e_hip {e_hip:.3e}  e_emul {e_emul:.3e}  ratio {e_hip / e_emul:.3f}  max|O - O_exact| / max|V| {worst:.4f}")
    assert e_hip <= R.REL_MARGIN * e_emul, (e_hip, e_emul)
    assert worst <= R.ABS_FRACTION, worst


@pytest.mark.parametrize("ns", [1, 2])
def test_mx_output_is_quantised_bf16_output(pkg, gpu, ns):
    c = R.Case(300, 200, 2, 4, ns)
    ops, _ = _case(c, _policy(pkg))
    o, oq, osc = _launch(pkg, gpu, ops, c.B, c.Sq, c.Sk, ns, mx_out=True)
    wq, ws = MX.quantize(o.reshape(-1, HD))
    assert torch.equal(osc, ws) and torch.equal(oq, _bits(wq))
    plain = _launch(pkg, gpu, ops, c.B, c.Sq, c.Sk, ns)
    assert torch.equal(plain, o), "the MX-writing launch changed the bf16 output"


# ------------------------------------------------------------------------------------------------ 4. model level
@pytest.fixture()
def every_site(pkg):
    """The goldens are small clips, where the engine's own rule (drn_attention_mxfp8_choice) keeps the bf16 attention: the
    model-level tests of the kernels switch every site to them."""
    was = pkg.native.attention_mxfp8_force(1)
    yield
    pkg.native.attention_mxfp8_force(was)


def test_small_clips_keep_the_bf16_attention(pkg, gpu):
    """The rule is a pure function of one clip's tokens; where it says 0 the switch changes no bit, sequencer and per-launch path."""
    Nn = pkg.native
    assert Nn.attention_mxfp8_force(-1) == 0
    assert [Nn.attention_mxfp8_choice(32, S) for S in (1, 256, 1024, 2047, 2048, 18432)] == [False, False, False, False, True, True]
    assert Nn.attention_mxfp8_choice(2, 2048) and not Nn.attention_mxfp8_choice(0, 4096)
    net, sd, x, cond = _tiny(pkg, gpu)
    t = torch.tensor(1.5)
    for precision in ("bf16", "mxfp8"):
        y0 = pkg.dit_engine.HipDiT(net, sd, device=gpu, precision=precision)(x, t, cond, [2, 4])
        on = pkg.dit_engine.HipDiT(net, sd, device=gpu, precision=precision, attention_precision="mxfp8")
        assert torch.equal(on(x, t, cond, [2, 4]), y0)
        on.trace = {}                                      # the per-launch path
        assert torch.equal(on(x, t, cond, [2, 4]), y0)
    was = Nn.attention_mxfp8_force(1)
    try:
        assert Nn.attention_mxfp8_choice(32, 256) and not torch.equal(on(x, t, cond, [2, 4]), y0)
    finally:
        Nn.attention_mxfp8_force(was)


def _model_inputs(pkg, meta, tag, net):
    sw = pkg.synthetic_weights
    F_, h, w = json.loads(meta["latent"])
    x = sw.synth_tensor(tag + ".x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(BF)
    cond = sw.synth_tensor(tag + ".cond", (1, net["additional_concat_ch"], F_, h, w), torch.float32, scale=1.0).to(BF)
    return x, cond, torch.tensor(float(meta["sigma"])), torch.full((1, 1), int(meta["context_index"]), dtype=torch.long)


@pytest.mark.parametrize("precision", ["bf16", "mxfp8"])
@pytest.mark.parametrize("fixture,tag,Dm,L,heads", [("dit_tinyA.safetensors", "tinyA", 256, 1, 2),
                                                    ("dit_tinyB.safetensors", "tinyB", 512, 2, 4)])
def test_model_matches_emulated_oracle(pkg, gpu, fixture, tag, Dm, L, heads, precision, every_site):
    from oracle import dit_oracle as O
    gold, meta = load_golden(fixture)
    net = tiny_net(pkg, Dm, L, heads)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF)
    x, cond, t, ci = _model_inputs(pkg, meta, tag, net)
    dit = pkg.dit_engine.HipDiT(net, {k: v.to(gpu) for k, v in sd.items()}, device=gpu, precision=precision,
                                attention_precision="mxfp8")
    y = dit(x.to(gpu), t.to(gpu), cond.to(gpu), ci.to(gpu)).float().cpu()
    torch.cuda.synchronize()
    # the oracle the emulated attention sits in carries the roundings of the engine around it: with MXFP8 linears the fp32 oracle
    # on quantise -> dequantise operands (as tests/test_mxfp8_gpu.py: that error dominates), with bf16 linears the bf16 oracle
    # that produced the golden's `out.bf16` (the engine rounds every activation to bf16 as it does; an fp32 oracle around the
    # emulated attention has less error than the bf16 reference itself, e_emul < e_ref, and is no stand-in for a bf16 engine)
    with torch.no_grad():
        if precision == "mxfp8":
            emul = R.mx_attn_mx_linear_oracle(O.DitOracle, _policy(pkg), heads)(sd, net, dtype=torch.float32,
                                                                               tables_dtype=BF).forward(x, t, cond, ci)
        else:
            emul = R.mx_attn_oracle(O.DitOracle, _policy(pkg), heads)(sd, net, dtype=BF).forward(x, t, cond, ci).float()
    exact = gold["out.fp32_tables_bf16"]
    e_ref, e_emul, e_hip = rel_l2(gold["out.bf16"], exact), rel_l2(emul, exact), rel_l2(y, exact)
    print(f"{tag} linears={precision} attention=mxfp8: e_ref={e_ref:.3e} e_emul={e_emul:.3e} ({e_emul / e_ref:.2f} x e_ref) "
          f"e_hip={e_hip:.3e} ({e_hip / e_ref:.2f} x e_ref)")
    assert e_hip <= 1.25 * e_emul, (e_hip, e_emul)


def test_full_28_blocks_cfg1_figure(pkg, gpu, every_site):
    """The 28-block model at cfg 1 with both switches on: print only (the figure of DESIGN 4c)."""
    gold, meta = load_golden("dit_full28_cfg1.safetensors")
    net = tiny_net(pkg, 4096, 28, 32)
    exact = gold["out.fp32_tables_bf16"]
    e_ref = rel_l2(gold["out.bf16"], exact)
    x, cond, t, ci = _model_inputs(pkg, meta, "full28", dict(net, additional_concat_ch=16))
    for precision in ("bf16", "mxfp8"):
        sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
        dit = pkg.dit_engine.HipDiT(net, sd, device=gpu, precision=precision, attention_precision="mxfp8")
        del sd
        torch.cuda.empty_cache()
        y = dit(x.to(gpu), t.to(gpu), cond.to(gpu), ci).float().cpu()
        e_hip = rel_l2(y, exact)
        print(f"full28 cfg1 linears={precision} attention=mxfp8: e_ref={e_ref:.3e} e_hip={e_hip:.3e} ({e_hip / e_ref:.2f} x e_ref)")
        assert torch.isfinite(y).all()
        del dit
        torch.cuda.empty_cache()


def _tiny(pkg, gpu, Dm=512, L=2, heads=4):
    net = tiny_net(pkg, Dm, L, heads)
    sd = {k: v.to(gpu) for k, v in pkg.synthetic_weights.synth_state_dict(net, BF).items()}
    sw = pkg.synthetic_weights
    x = sw.synth_tensor("mx.x", (2, 16, 2, 16, 16), torch.float32, scale=2.0).to(BF).to(gpu)
    cond = sw.synth_tensor("mx.c", (2, net["additional_concat_ch"], 2, 16, 16), torch.float32).to(BF).to(gpu)
    return net, sd, x, cond


@pytest.mark.parametrize("precision", ["bf16", "mxfp8"])
def test_sequencer_equals_per_launch_and_batch_invariant(pkg, gpu, monkeypatch, precision, every_site):
    net, sd, x, cond = _tiny(pkg, gpu)
    Hd = pkg.dit_engine.HipDiT
    monkeypatch.delenv("DRN_PER_LAUNCH", raising=False)
    seq = Hd(net, sd, device=gpu, precision=precision, attention_precision="mxfp8")
    monkeypatch.setenv("DRN_PER_LAUNCH", "1")
    per = Hd(net, sd, device=gpu, precision=precision, attention_precision="mxfp8")
    monkeypatch.delenv("DRN_PER_LAUNCH")
    assert per._per_launch and not seq._per_launch
    t = torch.tensor(1.5)
    ya = seq(x[:1], t, cond[:1], 2)
    assert torch.equal(ya, seq(x[:1], t, cond[:1], 2))
    assert torch.equal(ya, per(x[:1], t, cond[:1], 2))
    y2 = seq(x, t, cond, [2, 4])
    assert torch.equal(y2, per(x, t, cond, [2, 4]))
    assert torch.equal(y2[0:1], ya)
    assert torch.equal(y2[1:2], seq(x[1:2], t, cond[1:2], 4))
    # trace mode keeps the bf16 q and k (write_bf16) and the same result
    per.trace = {}
    assert torch.equal(per(x[:1], t, cond[:1], 2), ya)
    assert len(per.trace) == len(per.blocks) * len(per.kinds)
    per.trace = None
    base = Hd(net, sd, device=gpu, precision=precision)
    y0 = base(x[:1], t, cond[:1], 2)
    assert not torch.equal(ya, y0) and rel_l2(ya.cpu(), y0.cpu()) < 0.2


def test_default_unchanged_and_refusals(pkg, gpu, monkeypatch, every_site):
    net, sd, x, cond = _tiny(pkg, gpu)
    Hd = pkg.dit_engine.HipDiT
    monkeypatch.delenv("DRN_ATT_PRECISION", raising=False)
    monkeypatch.delenv("DRN_DIT_PRECISION", raising=False)
    t = torch.tensor(1.5)
    for precision in ("bf16", "mxfp8"):
        d0 = Hd(net, sd, device=gpu, precision=precision)
        d1 = Hd(net, sd, device=gpu, precision=precision, attention_precision="bf16")
        assert d0.attention_precision == "bf16" and not d0._amx and d0._mx_fused == (precision == "mxfp8") == d1._mx_fused
        y0 = d0(x[:1], t, cond[:1], 2)
        assert torch.equal(y0, d1(x[:1], t, cond[:1], 2))
    monkeypatch.setenv("DRN_ATT_PRECISION", "mxfp8")
    denv = Hd(net, sd, device=gpu)
    assert denv.attention_precision == "mxfp8" and denv.precision == "bf16"
    assert torch.equal(denv(x[:1], t, cond[:1], 2), Hd(net, sd, device=gpu, attention_precision="mxfp8")(x[:1], t, cond[:1], 2))
    monkeypatch.delenv("DRN_ATT_PRECISION")
    with pytest.raises(ValueError, match="unknown attention precision"):
        Hd(net, sd, device=gpu, attention_precision="fp4")
    with pytest.raises(ValueError, match="not built yet"):
        Hd(net, sd, device=gpu, attention_precision="mxfp8", process_group=object())
    assert pkg.dit_engine.PRECISIONS == ("bf16", "mxfp8") and pkg.dit_engine.ATTENTION_PRECISIONS == ("bf16", "mxfp8")
    m = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(
        dict(pkg.diffusion_renderer_config.get_inverse_renderer_config(), net=dict(net), dit_attention_precision="mxfp8"), device=gpu)
    full = dict(sd)
    full.update({k: torch.zeros(v, dtype=BF, device=gpu) for k, v in
                 {"logvar.0.freqs": (128,), "logvar.0.phases": (128,), "logvar.1.weight": (1, 128)}.items()})
    m.load_state_dict(full)
    assert m.net.attention_precision == "mxfp8" and m.net.precision == "bf16"


def test_loader_node_attention_precision(pkg, gpu, tmp_path, monkeypatch, every_site):
    import sys
    import types
    from safetensors.torch import save_file

    sw = pkg.synthetic_weights
    models = tmp_path / "models"
    vae_dir = models / "vae" / "Cosmos-1.0-Tokenizer-CV8x8x8" / "vae"
    vae_dir.mkdir(parents=True)
    (vae_dir / "config.json").write_text(json.dumps({**{k: (list(v) if isinstance(v, tuple) else v) for k, v in sw.COSMOS_CV8x8x8.items()},
                                                     "_class_name": "AutoencoderKLCosmos"}))
    save_file({k: v.contiguous() for k, v in sw.synth_vae_state_dict().items()}, str(vae_dir / "diffusion_pytorch_model.safetensors"))
    net = tiny_net(pkg, 256, 1, 2)
    ckpt_dir = models / "diffusion_models"
    ckpt_dir.mkdir()
    torch.save({"model": sw.synth_state_dict(net, BF)}, str(ckpt_dir / "tiny.pt"))
    fp = types.ModuleType("folder_paths")
    fp.models_dir = str(models)
    fp.get_filename_list = lambda kind: ["tiny.pt"] if kind == "diffusion_models" else []
    fp.get_full_path = lambda kind, name: str(models / kind / name)
    comfy = types.ModuleType("comfy")
    mm = types.ModuleType("comfy.model_management")
    mm.get_torch_device = lambda: gpu
    mm.soft_empty_cache = lambda: None
    cu = types.ModuleType("comfy.utils")
    cu.load_torch_file = lambda path, safe_load=False: torch.load(path, map_location="cpu", weights_only=True)
    comfy.model_management, comfy.utils = mm, cu
    for name, mod in (("folder_paths", fp), ("comfy", comfy), ("comfy.model_management", mm), ("comfy.utils", cu)):
        monkeypatch.setitem(sys.modules, name, mod)
    tiny_cfg = dict(pkg.diffusion_renderer_config.get_inverse_renderer_config(), net=dict(net))
    monkeypatch.setattr(pkg.nodes, "get_inverse_renderer_config", lambda *a, **k: dict(tiny_cfg))

    Loader = pkg.NODE_CLASS_MAPPINGS["LoadDiffusionRendererModel"]
    opt = Loader.INPUT_TYPES()["optional"]
    assert list(opt) == ["dit_precision", "attention_precision"]
    assert opt["attention_precision"][0] == ["bf16", "mxfp8"] and opt["attention_precision"][1]["default"] == "bf16"
    (pipe,) = Loader().load_pipeline("tiny.pt")
    assert pipe.pre_loaded_model_instance.net.attention_precision == "bf16"
    (pipe,) = Loader().load_pipeline("tiny.pt", attention_precision="mxfp8")
    assert pipe.pre_loaded_model_instance.net.attention_precision == "mxfp8"
    assert pipe.pre_loaded_model_instance.net.precision == "bf16"
    pipe.num_steps = 2
    image = sw.synth_tensor("ldr.img", (1, 9, 64, 64, 3), torch.float32).abs()
    outs = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(pipe, image, guidance=0.0, seed=42)
    assert len(outs) == 5 and all(o.shape == (9, 64, 64, 3) and torch.isfinite(o).all() for o in outs)
