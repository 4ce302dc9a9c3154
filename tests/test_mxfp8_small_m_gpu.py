"""MXFP8 at few tokens (csrc/gemm_mx_tall.hip, drn_dit_forward with precision 1): the lane maps of the few-token kernel with
exact integer data at every split count and both tile shapes, the kernel against the emulated product, the same bits through
every route (fused, sliced + reduce, sliced + the LayerNorm fold, stacked clips, repeated calls), the refusals, and the model on
the sequencer against the per-launch path and against the goldens with the small-M path switched off."""
import json

import pytest
import torch
import torch.nn.functional as F

import mx_emul as MX
from conftest import load_golden, rel_l2, tiny_net
from dit_refs import SENTINEL, is_sentinel

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CFG1 = [(12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384)]


def rnd(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF)


@pytest.fixture()
def small_m(pkg):
    """The small-M path on and the default tile shape, whatever an earlier test or the environment left; restored after."""
    lib = pkg.native.load_library()
    was = lib.drn_gemm_mxfp8_force_small_m(1)
    shape = lib.drn_gemm_mxfp8_tall_force_shape(-1)
    yield lib
    lib.drn_gemm_mxfp8_force_small_m(was)
    lib.drn_gemm_mxfp8_tall_force_shape(shape)


def _slices(pkg, a, w, splits, rows_per_batch=0):
    """fp32 slices [splits, M, N] of drn_gemm_mxfp8_splitk_partials."""
    lib = pkg.native.load_library()
    M, K = a.shape
    N = w.shape[0]
    ws = torch.empty((splits, M, N), dtype=torch.float32, device=a.q.device)
    assert ws.numel() * 4 == lib.drn_gemm_splitk_workspace_bytes(M, N, splits)
    rc = lib.drn_gemm_mxfp8_splitk_partials(a.q.data_ptr(), a.scales.data_ptr(), w.q.data_ptr(), w.scales.data_ptr(), M, N, K,
                                            rows_per_batch, splits, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return ws


# ------------------------------------------------------------------------------------------------ 1. lane maps
@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("N", [256, 512])
def test_small_m_lane_map_exact_integers(pkg, gpu, small_m, N, splits, shape):
    """The construction of test_mxfp8_gpu.test_gemm_lane_map_exact_integers on the few-token kernel: integers exact in e4m3
    (|a| <= 8, |w| <= 15), per-block scales 2^-1 .. 2^1, a row-dependent asymmetric W.  Every term is a multiple of 1/4 no larger
    than 16 x 30, so every partial sum is a multiple of 1/4 below 2^19: exact in fp32 in any order.  The bf16 output must equal
    the rounded exact product and the fp32 slices must sum (in fp64) to the exact product, at every split count, both shapes."""
    M, K = 256, 1024
    small_m.drn_gemm_mxfp8_tall_force_shape(shape)
    g = torch.Generator(device="cpu").manual_seed(5)
    ai = torch.randint(-8, 9, (M, K), generator=g).float()
    wi = torch.randint(-8, 9, (N, K), generator=g).float()
    wi[:, :K // 2] += torch.arange(N).view(N, 1).remainder(5)
    wi = wi.clamp(-15, 15)
    sa = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
    sw = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
    a = pkg.native.MxTensor(ai.to(torch.float8_e4m3fn).to(gpu), sa.to(gpu))
    w = pkg.native.MxTensor(wi.to(torch.float8_e4m3fn).to(gpu), sw.to(gpu))
    exact = (MX.dequantize(ai.to(torch.float8_e4m3fn), sa).double() @ MX.dequantize(wi.to(torch.float8_e4m3fn), sw).double().t())
    assert exact.abs().max() < 2 ** 18 and exact.to(BF).unique().numel() > 2000
    out = pkg.native.gemm_mxfp8(a, w, splitk=splits).cpu()
    ref = exact.to(BF)
    if not torch.equal(out, ref):
        bad = (out != ref).nonzero()
        pytest.fail(f"{bad.shape[0]} of {M * N} outputs differ; first (m, n): {bad[:8].tolist()}")
    if splits > 1:
        part = _slices(pkg, a, w, splits).cpu()
        assert torch.equal(part.double().sum(0), exact)
        # each slice is the exact product of its own K range
        Ks = K // splits
        da, dw = MX.dequantize(ai.to(torch.float8_e4m3fn), sa).double(), MX.dequantize(wi.to(torch.float8_e4m3fn), sw).double()
        for s in range(splits):
            assert torch.equal(part[s].double(), da[:, s * Ks:(s + 1) * Ks] @ dw[:, s * Ks:(s + 1) * Ks].t()), s


# ------------------------------------------------------------------------------------------------ 2. against the emulation
def _gemm_check(pkg, gpu, M, N, K, epi, splits, rows_per_batch=None, seed=0):
    """_gemm_check of test_mxfp8_gpu.py (quantise on the device, fp32 product of the dequantised operands as reference) through
    gemm_mxfp8(splitk=splits); clips stacked along the rows get one gate row each."""
    Nn = pkg.native
    a = rnd((M, K), 1.0, seed).to(gpu)
    w = rnd((N, K), K ** -0.5, seed + 1).to(gpu)
    aq, wq = Nn.mx_quant(a), Nn.mx_quant(w)
    lin = MX.dequantize(aq.q, aq.scales) @ MX.dequantize(wq.q, wq.scales).t()          # fp32 on the device
    # the output starts as NaN sentinels: a tile that is never written cannot pass on what the allocator's block held before
    fresh = torch.full((M, N), SENTINEL, dtype=torch.int16, device=gpu).view(BF)
    if epi == Nn.EPI_NONE:
        ref = lin
        out = Nn.gemm_mxfp8(aq, wq, out=fresh, rows_per_batch=rows_per_batch, splitk=splits)
    elif epi == Nn.EPI_GELU:
        ref = F.gelu(lin)
        out = Nn.gemm_mxfp8(aq, wq, out=fresh, epilogue=epi, rows_per_batch=rows_per_batch, splitk=splits)
    else:
        clips = M // rows_per_batch if rows_per_batch else 1
        gate = rnd((clips, N), 0.5, seed + 2).to(gpu)
        resid = rnd((M, N), 1.0, seed + 3).to(gpu)
        ref = resid.float() + (gate.float().view(clips, 1, N) * lin.view(clips, M // clips, N)).view(M, N)
        out = resid.clone()
        Nn.gemm_mxfp8(aq, wq, out=out, epilogue=epi, gate=gate, residual=out, rows_per_batch=rows_per_batch, splitk=splits)
    torch.cuda.synchronize()
    assert not bool(is_sentinel(out).any()), (M, N, K, epi, splits, "cells of the output were never written")
    e = rel_l2(out.float(), ref)
    print(f"mxfp8 small-M gemm M={M} rpb={rows_per_batch} N={N} K={K} epi={epi} splits={splits}: rel-L2 vs emulation {e:.2e}")
    assert e < 3e-3, (M, N, K, epi, splits, e)
    return e


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("N,K", CFG1 + [(256, 256), (512, 2048)])
@pytest.mark.parametrize("M,rpb", [(256, None), (512, None), (1024, None), (512, 256)])
def test_small_m_gemm_matches_emulation(pkg, gpu, small_m, M, rpb, N, K, epi):
    chosen = pkg.native.mx_gemm_plan(M, N, K, rpb)
    if chosen == 0:
        counts = [1, 2]
    else:
        counts = [chosen, 2 if chosen == 1 else chosen // 2]          # the chosen count and one forced different one
    for s in counts:
        assert (K // 128) % s == 0
        _gemm_check(pkg, gpu, M, N, K, epi, s, rows_per_batch=rpb, seed=M + N + K + epi)


def test_small_m_gemm_both_shapes_agree(pkg, gpu, small_m):
    """The two tile shapes run the same MFMA sequence per output element: same bits, fused and sliced."""
    Nn = pkg.native
    aq, wq = Nn.mx_quant(rnd((256, 4096), 1.0, 1).to(gpu)), Nn.mx_quant(rnd((4096, 4096), 4096 ** -0.5, 2).to(gpu))
    outs = []
    for shape in (0, 1):
        small_m.drn_gemm_mxfp8_tall_force_shape(shape)
        outs.append((Nn.gemm_mxfp8(aq, wq, epilogue=Nn.EPI_GELU, splitk=1), _slices(pkg, aq, wq, 4)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ 3. same bits through every route
def test_small_m_routes_give_the_same_bits(pkg, gpu, small_m):
    Nn = pkg.native
    lib = small_m
    D, K, S = 4096, 4096, 256
    st = lambda: torch.cuda.current_stream().cuda_stream
    splits = lib.drn_gemm_mxfp8_splitk_choice(S, D, K)
    assert splits > 1
    wq = Nn.mx_quant(rnd((D, K), K ** -0.5, 21).to(gpu))
    a2 = rnd((2 * S, K), 1.0, 22).to(gpu)
    x2 = rnd((2 * S, D), 1.0, 23).to(gpu)
    gate2 = rnd((2, D), 0.5, 24).to(gpu)
    shift2, scale2 = rnd((2, D), 0.3, 25).to(gpu), rnd((2, D), 0.3, 26).to(gpu)
    add2 = rnd((2, D), 0.2, 27).to(gpu)

    def fused_route(a, x, gate, shift, scale, add, rpb):
        """drn_gemm_mxfp8_splitk(GATE_RES) then drn_ln_modulate -> (x, h)"""
        x = x.clone()
        Nn.gemm_mxfp8(Nn.mx_quant(a), wq, out=x, epilogue=Nn.EPI_GATE_RES, gate=gate, residual=x, rows_per_batch=rpb, splitk=splits)
        h = Nn.ln_modulate(x, shift, scale, add_vec=add, rows_per_batch=rpb)
        return x, h

    def folded_route(a, x, gate, shift, scale, add, rpb):
        """drn_gemm_mxfp8_splitk_partials then drn_splitk_gate_res_ln_modulate -> (x, h)"""
        x = x.clone()
        h = torch.empty_like(x)
        part = _slices(pkg, Nn.mx_quant(a), wq, splits, rows_per_batch=rpb)
        rc = lib.drn_splitk_gate_res_ln_modulate(part.data_ptr(), splits, x.data_ptr(), gate.data_ptr(),
                                                 add.data_ptr() if add is not None else None, shift.data_ptr(), scale.data_ptr(),
                                                 h.data_ptr(), x.shape[0], D, rpb, 1e-6, st())
        assert rc == 0, rc
        return x, h

    for add in (None, add2):
        xa, ha = fused_route(a2, x2, gate2, shift2, scale2, add, S)
        xb, hb = folded_route(a2, x2, gate2, shift2, scale2, add, S)
        assert torch.equal(xa, xb) and torch.equal(ha, hb)
        # two runs of one call
        xc, hc = fused_route(a2, x2, gate2, shift2, scale2, add, S)
        assert torch.equal(xa, xc) and torch.equal(ha, hc)
        # the stacked clips, clip by clip, against the clips alone
        for b in range(2):
            r = slice(b * S, (b + 1) * S)
            ab = None if add is None else add[b:b + 1]
            x1, h1 = fused_route(a2[r], x2[r], gate2[b:b + 1], shift2[b:b + 1], scale2[b:b + 1], ab, S)
            assert torch.equal(x1, xa[r]) and torch.equal(h1, ha[r]), b
    # the unsplit kernel and the other epilogues: stacked == alone, run == run
    w2 = Nn.mx_quant(rnd((12288, K), K ** -0.5, 28).to(gpu))
    assert lib.drn_gemm_mxfp8_splitk_choice(S, 12288, K) == 1
    for epi in (Nn.EPI_NONE, Nn.EPI_GELU):
        y2 = Nn.gemm_mxfp8(Nn.mx_quant(a2), w2, epilogue=epi, rows_per_batch=S)
        assert torch.equal(y2, Nn.gemm_mxfp8(Nn.mx_quant(a2), w2, epilogue=epi, rows_per_batch=S))
        for b in range(2):
            r = slice(b * S, (b + 1) * S)
            assert torch.equal(y2[r], Nn.gemm_mxfp8(Nn.mx_quant(a2[r]), w2, epilogue=epi))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_small_m_refusals(pkg, gpu, small_m):
    Nn = pkg.native
    lib = small_m
    st = torch.cuda.current_stream().cuda_stream
    a = Nn.mx_quant(rnd((512, 1024)).to(gpu))
    w = Nn.mx_quant(rnd((512, 1024), 0.03, 1).to(gpu))
    out = torch.full((512, 512), 7.0, dtype=BF, device=gpu)
    ws = torch.zeros(64 * 512 * 512, dtype=torch.float32, device=gpu)

    def call(M=256, N=512, K=1024, splits=2, wsp=ws.data_ptr()):
        return lib.drn_gemm_mxfp8_splitk(a.q.data_ptr(), a.scales.data_ptr(), w.q.data_ptr(), w.scales.data_ptr(), out.data_ptr(),
                                         M, N, K, 512, 0, None, None, 0, 0, splits, wsp, st)

    assert call(M=256 + 64) == -1                 # M % 256
    assert call(splits=3) == -1                   # does not divide K / 128 = 8
    assert call(splits=128) == -1 and call(splits=65) == -1          # > 64
    assert call(wsp=None) == -1                   # slices without a workspace
    assert lib.drn_gemm_mxfp8_splitk_partials(a.q.data_ptr(), a.scales.data_ptr(), w.q.data_ptr(), w.scales.data_ptr(),
                                              256 + 64, 512, 1024, 0, 2, ws.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0).all())        # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out[:256] == 7.0).all()) and bool((out[256:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ 5. model
def _inputs(pkg, gpu, net, tag, B, latent):
    sw = pkg.synthetic_weights
    F_, h, w = latent
    x = sw.synth_tensor(tag + ".x", (B, 16, F_, h, w), torch.float32, scale=2.0).to(BF).to(gpu)
    cond = sw.synth_tensor(tag + ".c", (B, net["additional_concat_ch"], F_, h, w), torch.float32).to(BF).to(gpu)
    return x, cond


@pytest.mark.parametrize("tag,D,L,heads,latent", [("tinyB", 512, 2, 4, (2, 16, 16)), ("wide1", 4096, 1, 32, (1, 32, 32))])
def test_mxfp8_sequencer_equals_per_launch(pkg, gpu, small_m, monkeypatch, tag, D, L, heads, latent):
    """An mxfp8 engine on drn_dit_forward and one built under DRN_PER_LAUNCH=1 issue the same launches: same bits.  tinyB
    (S = 128) is below every small-M rule; wide1 (D = 4096, S = 256) runs the few-token kernel, its slices and the deferred
    LayerNorm fold; a two-clip batch of it reproduces each clip alone."""
    net = tiny_net(pkg, D, L, heads)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
    S = latent[0] * (latent[1] // 2) * (latent[2] // 2)
    plans = [pkg.native.mx_gemm_plan(S, n, k) for n, k in [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]]
    if tag == "tinyB":
        assert S == 128 and plans == [0, 0, 0, 0]
    else:
        assert S == 256 and min(plans) >= 1 and plans[1] > 1 and plans[3] > 1
    H = pkg.dit_engine.HipDiT
    monkeypatch.delenv("DRN_PER_LAUNCH", raising=False)
    seq = H(net, sd, device=gpu, precision="mxfp8")
    monkeypatch.setenv("DRN_PER_LAUNCH", "1")
    per = H(net, sd, device=gpu, precision="mxfp8")
    monkeypatch.delenv("DRN_PER_LAUNCH")
    assert not seq._per_launch and per._per_launch
    x, cond = _inputs(pkg, gpu, net, "mxs." + tag, 2, latent)
    t = torch.tensor(1.5)
    y1 = seq(x[:1], t, cond[:1], 2)
    assert torch.isfinite(y1).all()
    assert torch.equal(y1, per(x[:1], t, cond[:1], 2))
    assert torch.equal(y1, seq(x[:1], t, cond[:1], 2))
    y2 = seq(x, t, cond, [2, 4])
    assert torch.equal(y2, per(x, t, cond, [2, 4]))
    assert torch.equal(y2[0:1], y1)
    assert torch.equal(y2[1:2], seq(x[1:2], t, cond[1:2], 4))
    if tag == "wide1":
        # the small-M path is live: switching it off changes the summation order, not the result beyond the mxfp8 noise
        small_m.drn_gemm_mxfp8_force_small_m(0)
        y0 = seq(x[:1], t, cond[:1], 2)
        small_m.drn_gemm_mxfp8_force_small_m(1)
        assert not torch.equal(y0, y1) and rel_l2(y1.cpu(), y0.cpu()) < 2e-2


def test_mxfp8_full_28_blocks_small_m_against_hook_off(pkg, gpu, small_m):
    """The 28-block model in mxfp8 at cfg 1 (S = 256) and S = 1024 against the goldens, on one engine: once with the small-M
    path off (the kernels an mxfp8 engine ran before it existed: the reference) and once with it on.  Only the fp32 summation
    order differs, so e_mx_hip must stay within the 1.25 the mxfp8 model test gives the HIP path over its reference."""
    net = tiny_net(pkg, 4096, 28, 32)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
    dit = pkg.dit_engine.HipDiT(net, sd, device=gpu, precision="mxfp8")
    del sd
    torch.cuda.empty_cache()
    sw = pkg.synthetic_weights
    for fixture, tag in [("dit_full28_cfg1.safetensors", "full28"), ("dit_full28_s1024.safetensors", "full28_s1024")]:
        gold, meta = load_golden(fixture)
        F_, h, w = json.loads(meta["latent"])
        x = sw.synth_tensor(tag + ".x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(BF)
        cond = sw.synth_tensor(tag + ".cond", (1, 16, F_, h, w), torch.float32, scale=1.0).to(BF)
        t = torch.tensor(float(meta["sigma"]))
        ci = torch.full((1, 1), int(meta["context_index"]), dtype=torch.long)
        exact = gold["out.fp32_tables_bf16"]
        e = {}
        for on in (1, 0):                         # on first: the workspace of a shape is sized under the setting it is built with
            small_m.drn_gemm_mxfp8_force_small_m(on)
            y = dit(x.to(gpu), t, cond.to(gpu), ci).float().cpu()
            assert torch.isfinite(y).all()
            e[on] = rel_l2(y, exact)
        small_m.drn_gemm_mxfp8_force_small_m(1)
        e_ref = rel_l2(gold["out.bf16"], exact)
        print(f"{tag}: e_ref={e_ref:.3e} e_mx_hip(hook off)={e[0]:.3e} e_mx_hip(small-M)={e[1]:.3e} ({e[1] / e[0]:.3f} x)")
        assert e[1] <= 1.25 * e[0], (tag, e)
    del dit
    torch.cuda.empty_cache()
