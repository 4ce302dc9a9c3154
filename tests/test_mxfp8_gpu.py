"""MXFP8 block linears (HipDiT(precision="mxfp8"), include/drn.h): quantiser bit for bit against the torch emulation
(tests/mx_emul.py), the scaled MFMA's lane maps with exact integer data, the GEMM against the emulated product, the model
against the goldens with the fp32 oracle on emulated MXFP8 block linears, the default path unchanged, determinism, refusals
and the loader node."""
import json

import pytest
import torch
import torch.nn.functional as F

import mx_emul as MX
from conftest import load_golden, rel_l2, tiny_net
from dit_refs import SENTINEL, is_sentinel

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def rnd(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF)


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


# ------------------------------------------------------------------------------------------------ 1. quantiser, bit-exact
def _quant_cases():
    g = torch.Generator(device="cpu").manual_seed(11)
    rows = []
    rows.append(torch.randn(64, 512, generator=g) * 3.0)                             # random
    x = torch.randn(32, 512, generator=g) * 0.01
    x.view(32, 16, 32)[:, :, 7] = 300.0 * (torch.rand(32, 16, generator=g) + 0.5)    # one large outlier per block
    rows.append(x)
    m = torch.randn(8, 512, generator=g).clamp(-1.0, 1.0)
    m.view(8, 16, 32)[:, ::2, 3] = 1.75 * 2.0 ** torch.arange(-4, 4).float().view(8, 1)           # significand exactly 1.75
    m.view(8, 16, 32)[:, 1::2, 5] = -(1.75 + 2 ** -7) * 2.0 ** torch.arange(-4, 4).float().view(8, 1)   # just above 1.75
    rows.append(m)
    z = torch.randn(8, 512, generator=g)
    z.view(8, 16, 32)[:, ::3] = 0.0                                                 # all-zero blocks
    rows.append(z)
    s = torch.randn(8, 512, generator=g) * 2.0 ** -128                              # bf16 subnormals
    s.view(8, 16, 32)[:, 1::2] *= 2.0 ** 10                                         # and small normals beside them
    rows.append(s)
    big = torch.randn(4, 512, generator=g) * 2.0 ** 100                             # large exponents
    rows.append(big)
    return torch.cat(rows, 0).to(BF)


def test_quantiser_bit_exact(pkg, gpu):
    x = _quant_cases()
    ref_q, ref_s = MX.quantize(x)
    got = pkg.native.mx_quant(x.to(gpu))
    assert torch.equal(_bits(got.scales), ref_s)
    assert torch.equal(_bits(got.q), _bits(ref_q)), f"{(_bits(got.q) != _bits(ref_q)).sum().item()} element bytes differ"
    assert int(ref_s.min()) >= 0 and int(ref_s.max()) <= 254


def test_quantiser_strided_input(pkg, gpu):
    base = rnd((300, 1024 + 64), 2.0, seed=3)
    x = base.to(gpu)[:, 32:32 + 1024]                          # row stride 1088, 64-byte offset
    ref_q, ref_s = MX.quantize(base[:, 32:32 + 1024].contiguous())
    got = pkg.native.mx_quant(x)
    assert torch.equal(_bits(got.scales), ref_s)
    assert torch.equal(_bits(got.q), _bits(ref_q))


# ------------------------------------------------------------------------------------------------ 2. lane maps
def test_gemm_lane_map_exact_integers(pkg, gpu):
    """Small integers (exact in e4m3) with per-block scales 2^-1 .. 2^1 on both operands and an asymmetric W: every partial sum
    is exact in fp32, so the bf16 output must equal the rounded integer product exactly.  A wrong operand, K or scale lane map
    (or swapped C rows / columns) changes the result."""
    M, N, K = 48, 256, 512
    g = torch.Generator(device="cpu").manual_seed(5)
    ai = torch.randint(-8, 9, (M, K), generator=g).float()
    wi = torch.randint(-8, 9, (N, K), generator=g).float()
    wi[:, :K // 2] += torch.arange(N).view(N, 1).remainder(5)        # asymmetric: W != W^T structure, row-dependent
    wi = wi.clamp(-15, 15)
    sa = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
    sw = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
    a = pkg.native.MxTensor(ai.to(torch.float8_e4m3fn).to(gpu), sa.to(gpu))
    w = pkg.native.MxTensor(wi.to(torch.float8_e4m3fn).to(gpu), sw.to(gpu))
    out = pkg.native.gemm_mxfp8(a, w).cpu()
    exact = (MX.dequantize(ai.to(torch.float8_e4m3fn), sa).double() @ MX.dequantize(wi.to(torch.float8_e4m3fn), sw).double().t())
    ref = exact.to(BF)
    if not torch.equal(out, ref):
        bad = (out != ref).nonzero()
        pytest.fail(f"{bad.shape[0]} of {M * N} outputs differ; first (m, n): {bad[:8].tolist()}")


# ------------------------------------------------------------------------------------------------ 3. GEMM vs emulation
def _gemm_check(pkg, gpu, M, N, K, epi, seed=0):
    Nn = pkg.native
    a = rnd((M, K), 1.0, seed).to(gpu)
    w = rnd((N, K), K ** -0.5, seed + 1).to(gpu)
    aq, wq = Nn.mx_quant(a), Nn.mx_quant(w)
    lin = MX.dequantize(aq.q, aq.scales) @ MX.dequantize(wq.q, wq.scales).t()          # fp32 on the device
    gate = resid = None
    # the output starts as NaN sentinels: a tile that is never written cannot pass on what the allocator's block held before
    fresh = torch.full((M, N), SENTINEL, dtype=torch.int16, device=gpu).view(BF)
    if epi == Nn.EPI_NONE:
        ref = lin
        out = Nn.gemm_mxfp8(aq, wq, out=fresh)
    elif epi == Nn.EPI_GELU:
        ref = F.gelu(lin)
        out = Nn.gemm_mxfp8(aq, wq, out=fresh, epilogue=epi)
    else:
        gate = rnd((1, N), 0.5, seed + 2).to(gpu)
        resid = rnd((M, N), 1.0, seed + 3).to(gpu)
        ref = resid.float() + gate.float() * lin
        out = resid.clone()
        Nn.gemm_mxfp8(aq, wq, out=out, epilogue=epi, gate=gate, residual=out)
    torch.cuda.synchronize()
    assert not bool(is_sentinel(out).any()), (M, N, K, epi, "cells of the output were never written")
    e = rel_l2(out.float(), ref)
    assert e < 3e-3, (M, N, K, epi, e)
    return e


@pytest.mark.parametrize("M", [1, 100, 256, 2048 + 37])
@pytest.mark.parametrize("N,K", [(768, 256), (256, 256), (1024, 256), (256, 1024), (1536, 512), (512, 2048)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_mxfp8_small_shapes(pkg, gpu, M, N, K, epi):
    _gemm_check(pkg, gpu, M, N, K, epi, seed=M + N + K + epi)


@pytest.mark.parametrize("N,K,epi", [(12288, 4096, 0), (4096, 4096, 2), (16384, 4096, 1), (4096, 16384, 2)])
@pytest.mark.parametrize("M", [100, 18432])
def test_gemm_mxfp8_cfg3_shapes(pkg, gpu, M, N, K, epi):
    e = _gemm_check(pkg, gpu, M, N, K, epi, seed=7)
    print(f"mxfp8 gemm M={M} N={N} K={K} epi={epi}: rel-L2 vs emulation {e:.2e}")


def test_gemm_mxfp8_rejects_bad_shapes(pkg, gpu):
    Nn = pkg.native
    a = Nn.mx_quant(rnd((64, 256)).to(gpu))
    with pytest.raises(ValueError):
        Nn.gemm_mxfp8(a, Nn.mx_quant(rnd((128, 256)).to(gpu)))          # N % 256
    with pytest.raises(ValueError):
        Nn.gemm_mxfp8(Nn.mx_quant(rnd((64, 96)).to(gpu)), Nn.mx_quant(rnd((256, 96)).to(gpu)))    # K % 128
    lib = Nn.load_library()
    assert lib.drn_gemm_mxfp8(a.q.data_ptr(), a.scales.data_ptr(), a.q.data_ptr(), a.scales.data_ptr(), a.q.data_ptr(),
                              64, 128, 256, 256, 0, None, None, 0, 64, None) == -1


# ------------------------------------------------------------------------------------------------ 4. model vs goldens
def _model_inputs(pkg, meta, tag, net):
    sw = pkg.synthetic_weights
    F_, h, w = json.loads(meta["latent"])
    x = sw.synth_tensor(tag + ".x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(BF)
    cond = sw.synth_tensor(tag + ".cond", (1, net["additional_concat_ch"], F_, h, w), torch.float32, scale=1.0).to(BF)
    return x, cond, torch.tensor(float(meta["sigma"])), torch.full((1, 1), int(meta["context_index"]), dtype=torch.long)


@pytest.mark.parametrize("fixture,tag,D,L,heads", [("dit_tinyA.safetensors", "tinyA", 256, 1, 2),
                                                   ("dit_tinyB.safetensors", "tinyB", 512, 2, 4),
                                                   ("dit_wide1.safetensors", "wide1", 4096, 1, 32)])
def test_mxfp8_model_matches_emulated_oracle(pkg, gpu, fixture, tag, D, L, heads):
    from oracle import dit_oracle as O
    gold, meta = load_golden(fixture)
    net = tiny_net(pkg, D, L, heads)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF)
    x, cond, t, ci = _model_inputs(pkg, meta, tag, net)
    dit = pkg.dit_engine.HipDiT(net, {k: v.to(gpu) for k, v in sd.items()}, device=gpu, precision="mxfp8")
    y = dit(x.to(gpu), t.to(gpu), cond.to(gpu), ci.to(gpu)).float().cpu()
    torch.cuda.synchronize()
    with torch.no_grad():
        emul = MX.mx_oracle(O.DitOracle)(sd, net, dtype=torch.float32, tables_dtype=BF).forward(x, t, cond, ci)
    exact = gold["out.fp32_tables_bf16"]
    e_ref, e_emul, e_hip, d = rel_l2(gold["out.bf16"], exact), rel_l2(emul, exact), rel_l2(y, exact), rel_l2(y, emul)
    print(f"{tag}: e_ref={e_ref:.3e} e_mx_emul={e_emul:.3e} e_mx_hip={e_hip:.3e} rel-L2(hip, emul)={d:.3e}")
    assert e_hip <= 1.25 * e_emul, (e_hip, e_emul)


def test_mxfp8_full_28_blocks_cfg1(pkg, gpu):
    """The 28-block model at cfg 1 (S = 256) in mxfp8 (its own instance: the session's bf16 one stays as it is).  The fp32
    emulated oracle of 7.2 B parameters is not run here (CPU time); the figure is printed next to the bf16 ones."""
    gold, meta = load_golden("dit_full28_cfg1.safetensors")
    net = tiny_net(pkg, 4096, 28, 32)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
    dit = pkg.dit_engine.HipDiT(net, sd, device=gpu, precision="mxfp8")
    del sd
    torch.cuda.empty_cache()
    x, cond, t, ci = _model_inputs(pkg, meta, "full28", dict(net, additional_concat_ch=16))
    y = dit(x.to(gpu), t.to(gpu), cond.to(gpu), ci).float().cpu()
    exact = gold["out.fp32_tables_bf16"]
    e_ref, e_hip = rel_l2(gold["out.bf16"], exact), rel_l2(y, exact)
    print(f"full28 cfg1: e_ref={e_ref:.3e} e_mx_hip={e_hip:.3e} ({e_hip / e_ref:.2f} x e_ref)")
    assert torch.isfinite(y).all()
    del dit
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 5-7. default, determinism, refusal
def _tiny(pkg, gpu, D=512, L=2, heads=4):
    net = tiny_net(pkg, D, L, heads)
    sd = {k: v.to(gpu) for k, v in pkg.synthetic_weights.synth_state_dict(net, BF).items()}
    sw = pkg.synthetic_weights
    x = sw.synth_tensor("mx.x", (2, 16, 2, 16, 16), torch.float32, scale=2.0).to(BF).to(gpu)
    cond = sw.synth_tensor("mx.c", (2, net["additional_concat_ch"], 2, 16, 16), torch.float32).to(BF).to(gpu)
    return net, sd, x, cond


def test_bf16_default_unchanged(pkg, gpu, monkeypatch):
    net, sd, x, cond = _tiny(pkg, gpu)
    H = pkg.dit_engine.HipDiT
    monkeypatch.delenv("DRN_DIT_PRECISION", raising=False)
    y0 = H(net, sd, device=gpu)(x[:1], torch.tensor(1.5), cond[:1], 2)
    y1 = H(net, sd, device=gpu, precision="bf16")(x[:1], torch.tensor(1.5), cond[:1], 2)
    monkeypatch.setenv("DRN_DIT_PRECISION", "bf16")
    y2 = H(net, sd, device=gpu)(x[:1], torch.tensor(1.5), cond[:1], 2)
    monkeypatch.delenv("DRN_DIT_PRECISION")
    m = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(
        dict(pkg.diffusion_renderer_config.get_inverse_renderer_config(), net=dict(net), dit_precision="bf16"), device=gpu)
    full = dict(sd)
    full.update({k: torch.zeros(v, dtype=BF, device=gpu) for k, v in
                 {"logvar.0.freqs": (128,), "logvar.0.phases": (128,), "logvar.1.weight": (1, 128)}.items()})
    m.load_state_dict(full)
    assert m.net.precision == "bf16"
    y3 = m.net(x[:1], torch.tensor(1.5), cond[:1], 2)
    for y in (y1, y2, y3):
        assert torch.equal(y, y0)
    monkeypatch.setenv("DRN_DIT_PRECISION", "mxfp8")
    dmx = H(net, sd, device=gpu)
    assert dmx.precision == "mxfp8"
    ymx = dmx(x[:1], torch.tensor(1.5), cond[:1], 2)
    assert not torch.equal(ymx, y0) and rel_l2(ymx.cpu(), y0.cpu()) < 0.2


def test_mxfp8_deterministic_and_batch_invariant(pkg, gpu):
    net, sd, x, cond = _tiny(pkg, gpu)
    dit = pkg.dit_engine.HipDiT(net, sd, device=gpu, precision="mxfp8")
    ya = dit(x[:1], torch.tensor(1.5), cond[:1], 2)
    yb = dit(x[:1], torch.tensor(1.5), cond[:1], 2)
    assert torch.equal(ya, yb)
    y2 = dit(x, torch.tensor(1.5), cond, [2, 4])
    assert torch.equal(y2[0:1], ya)
    assert torch.equal(y2[1:2], dit(x[1:2], torch.tensor(1.5), cond[1:2], 4))


def test_mxfp8_refusals(pkg, gpu):
    net, sd, _, _ = _tiny(pkg, gpu, 256, 1, 2)
    H = pkg.dit_engine.HipDiT
    with pytest.raises(ValueError, match="not built yet"):
        H(net, sd, device=gpu, precision="mxfp8", process_group=object())
    with pytest.raises(ValueError, match="unknown DiT precision"):
        H(net, sd, device=gpu, precision="fp4")


# ------------------------------------------------------------------------------------------------ 8. loader node
def test_loader_node_mxfp8(pkg, gpu, tmp_path, monkeypatch):
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
    opt = Loader.INPUT_TYPES()["optional"]["dit_precision"]
    assert opt[0] == ["bf16", "mxfp8"] and opt[1]["default"] == "bf16"
    (pipe,) = Loader().load_pipeline("tiny.pt", dit_precision="mxfp8")
    assert pipe.pre_loaded_model_instance.net.precision == "mxfp8"
    pipe.num_steps = 2
    image = sw.synth_tensor("ldr.img", (1, 9, 64, 64, 3), torch.float32).abs()
    outs = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(pipe, image, guidance=0.0, seed=42)
    assert len(outs) == 5 and all(o.shape == (9, 64, 64, 3) and torch.isfinite(o).all() for o in outs)
