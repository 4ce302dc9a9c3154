"""Tokenizer kernels (csrc/conv_igemm.hip, conv256s.hip, vae_kernels.hip) held to ulp-level parity at the model's shapes.

Every kernel is compared with an fp64 reference built from the same bf16 inputs (tests/vae_refs.py: the kernels' documented
rounding points and nothing else), bit for bit where the arithmetic allows it (exact-integer convolutions, index moves), in
bf16 ulps with a floor on the share of bit-equal elements elsewhere.  tests/test_vae_refs_cpu.py shows without a GPU that every
bound used here passes a correct bf16 implementation and fails subtly wrong ones.  Each case prints one `tokenizer-kernel` line
with its figures (collected by tools/gpu_parity.sh).

GroupNorm, measured on MI355X: with the variance formed from sums already cast to fp32 (the kernel before this module existed)
all four offset-frame cases failed on the bit-equal share (0.886 .. 0.932 against torch's 0.991 .. 0.995); with mean, variance and
rstd formed from the fp64 sums they pass (0.9946 .. 0.9982).  All figures: profiles/tokenizer_kernel_parity.txt.
"""
import math

import pytest
import torch

import vae_refs as R
from oracle import vae_oracle as VO

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def say(tag, res=None, extra=""):
    print(f"tokenizer-kernel {tag}: {R.fmt(res) if res is not None else ''}{extra}")


def to_cl(V, x, gpu, halo=1, Cs=None):
    """[C, T, H, W] cpu bf16 -> CL on the gpu (Cs stored channels, zero tail and halo)."""
    C, T, H, W = x.shape
    cl = V.CL(T, H, W, Cs or C, halo, gpu, tensor=torch.zeros((T, H + 2 * halo, W + 2 * halo, Cs or C), dtype=BF, device=gpu))
    cl.interior()[..., :C].copy_(x.permute(1, 2, 3, 0).to(gpu))
    return cl


def stored(y, Cs, halo):
    """[C, T, H, W] cpu bf16 -> the whole stored tensor [T, H + 2 halo, W + 2 halo, Cs] with zero tail and halo."""
    C, T, H, W = y.shape
    out = torch.zeros((T, H + 2 * halo, W + 2 * halo, Cs), dtype=BF)
    out[:, halo:halo + H, halo:halo + W, :C] = y.permute(1, 2, 3, 0)
    return out


def repack(w, gpu):
    co, ci, kt, kh, kw = w.shape
    return w.permute(0, 2, 3, 4, 1).reshape(co, kt * kh * kw * ci).contiguous().to(gpu)


# ------------------------------------------------------------------------------------------------ convolution
def run_conv(pkg, gpu, g, x, w, b, res, tile):
    """One launch of geometry g on the 128 x 128 kernel (tile 0) or with the streamed kernel forced (tile 1).  Returns the whole
    stored output (CPU) and which kernel ran."""
    V = pkg.native_vae
    lib = pkg.native.load_library()
    xc = to_cl(V, x, gpu, g.in_halo)
    rc = None
    if g.res == "input":
        rc = xc
    elif g.res is not None:
        rc = to_cl(V, res, gpu, g.out_halo, g.cs)
    lib.drn_conv_force_tile(tile)
    try:
        y = V.conv3d(xc, repack(w, gpu), b.to(gpu), g.cout, g.k, g.stride, g.pad, g.t_off, out=rc if g.res == "output" else None,
                     residual=rc, out_halo=g.out_halo, out_dims=R.conv_out_dims(g, *x.shape[1:]), out_channels_stored=g.cs)
        ran = lib.drn_conv_last_tile()
    finally:
        lib.drn_conv_force_tile(-1)
    if g.res == "input":
        assert torch.equal(xc.interior().permute(3, 0, 1, 2).cpu(), x), "the input that doubles as residual was modified"
    return y.t.cpu(), ran


@pytest.fixture(scope="module")
def recorded(pkg, gpu):
    """The geometry of every conv launch of one encode + decode of a (9, 32, 48) clip."""
    V = pkg.native_vae
    sw = pkg.synthetic_weights
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    names = {w[0].data_ptr(): name for name, w in vae.model.w.items()}
    clip = sw.synth_tensor("kernels.clip", (1, 3, 9, 32, 48), torch.float32, device=gpu).to(BF)
    with R.record_convs(V, names) as rec:
        vae.decode(vae.encode(clip))
    torch.cuda.synchronize()
    return rec


def test_recorder_saw_every_conv_weight_of_the_tokenizer(pkg, recorded):
    want = {n[:-7] for n, s in pkg.synthetic_weights.vae_param_shapes().items() if n.endswith(".weight") and len(s) == 5}
    assert want and want <= recorded.seen, sorted(want - recorded.seen)[:5]
    say("recorder", extra=f"{len(recorded.geoms)} distinct conv geometries over {sum(map(len, recorded.geoms.values()))} launches")
    kinds = {g.res for g in recorded.geoms}
    assert {None, "fresh", "input"} <= kinds, kinds
    assert any(g.out_halo == 0 for g in recorded.geoms) and any(g.in_halo == 0 for g in recorded.geoms)
    assert any(g.cs > g.cout for g in recorded.geoms) and {192, 512} <= {g.cin for g in recorded.geoms}


def test_conv_exact_integers_every_geometry(pkg, gpu, recorded):
    """Integer activations / weights / bias / residual: every partial sum is an integer below 2^24, so fp32 accumulation is
    exact in any order and the WHOLE stored output (zero channel tail and zero halo included) must equal the reference bit for
    bit, both bf16 roundings included - on the 128 x 128 kernel and on the streamed kernel wherever it runs.  A wrong tap order,
    clamp, stride origin, halo offset, channel tail or C-fragment map changes integers."""
    geoms = list(dict.fromkeys(list(recorded.geoms) + R.conv_edge_geoms()))
    bad, launches, streamed = [], 0, 0
    for gi, g in enumerate(geoms):
        for T, H, W in R.conv_sizes(g):
            x, w, b, res = R.conv_inputs(g, T, H, W, True, seed=11 + gi)
            ref, _ = R.conv_ref(g, x, w, b, res, T, H, W)
            want = stored(ref.to(BF), g.cs, g.out_halo)
            for tile in (0, 1):
                got, ran = run_conv(pkg, gpu, g, x, w, b, res, tile)
                if tile == 0:
                    assert ran == 0
                elif ran != 1:
                    continue
                launches += 1
                streamed += ran
                if not torch.equal(got, want):
                    inner = (got != want).sum().item()
                    bad.append(f"{g} T{T} H{H} W{W} kernel {ran}: {inner} of {want.numel()} stored elements differ")
    say("conv exact integers", extra=f"{len(geoms)} geometries, {launches} launches ({streamed} streamed), {len(bad)} not bit-equal")
    assert streamed > 0
    assert not bad, "\n".join(bad)


def test_conv_random_data_model_channel_counts(pkg, gpu):
    """Random bf16 data at the tokenizer's channel counts against the fp64 reference: the bound of the MFMA GEMM tests (1 ulp,
    atol 2e-3 rms, >= 0.98 bit-equal; with a residual 2 ulp of max(|conv|, |res|) and >= 0.97); both kernels bit-identical."""
    bad = []
    for tag, g, live in R.conv_model_cases():
        T, H, W = R.conv_model_size(g)
        x, w, b, res = R.conv_inputs(g, T, H, W, False, seed=R.CONV_MODEL_SEED, cin_live=live)
        ref, mag = R.conv_ref(g, x, w, b, res, T, H, W)
        got, _ = run_conv(pkg, gpu, g, x, w, b, res, 0)
        got1, ran = run_conv(pkg, gpu, g, x, w, b, res, 1)
        h = g.out_halo
        interior = got[:, h:h + ref.shape[2], h:h + ref.shape[3], :g.cout].permute(3, 0, 1, 2)
        r = R.ulp_check(interior, ref, mag=mag, max_ulp=2 if res is not None else 1, frac_exact=0.97 if res is not None else 0.98)
        say(f"conv {tag}", r, f"  streamed kernel ran: {ran == 1}")
        if not r["ok"]:
            bad.append((tag, R.fmt(r)))
        if not torch.equal(got, stored(interior, g.cs, h)):
            bad.append((tag, "channel tail or halo of the stored output is not zero"))
        if ran == 1 and not torch.equal(got, got1):
            bad.append((tag, "streamed kernel differs from the 128 x 128 kernel"))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ GroupNorm
def _gn_run(pkg, gpu, x, gm, bt, silu):
    V = pkg.native_vae
    y = V.groupnorm_silu(to_cl(V, x, gpu), gm.to(gpu), bt.to(gpu), silu)
    return y.t.cpu()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C,H,W", R.GN_CASES)
def test_groupnorm_every_thread_map(pkg, gpu, C, H, W, silu):
    """Row kernel (C = 128, 256, 512) and generic kernel (192, 320), four frames with different mean and scale, whole stored
    tensor.  Without SiLU the LayerNorm tests' bound; with SiLU at most twice torch's own bf16 mismatch share + 1e-3."""
    x, gm, bt = R.gn_inputs(C, H, W, "centred")
    ref = R.gn_ref(x, gm, bt, silu)
    got = _gn_run(pkg, gpu, x, gm, bt, silu)
    interior = got[:, 1:1 + H, 1:1 + W].permute(3, 0, 1, 2)
    assert torch.equal(got, stored(interior, C, 1)), "halo written"
    if not silu:
        r = R.ulp_check(interior, ref, max_ulp=1, frac_exact=0.995)
        say(f"groupnorm C{C} {H}x{W}", r)
        assert r["ok"], R.fmt(r)
        return
    t = R.ulp_check(R.gn_torch_bf16(x, gm, bt, True), ref, max_ulp=1, frac_exact=0.0)
    r = R.ulp_check(interior, ref, max_ulp=1, frac_exact=0.0)
    say(f"groupnorm+silu C{C} {H}x{W}", r, f"  torch bf16: exact {t['exact']:.5f}")
    assert r["bad"] == 0, R.fmt(r)
    assert 1 - r["exact"] <= 2 * (1 - t["exact"]) + 1e-3, (r["exact"], t["exact"])


@pytest.mark.parametrize("C,H,W", R.GN_OFFSET_CASES)
def test_groupnorm_offset_frames(pkg, gpu, C, H, W):
    """Frames whose mean is 32 .. 250 times their spread (64 + 0.5 z, 256 + 2 z, 1000 + 4 z, -16 + 0.5 z): q / n - mean^2 cancels
    unless it is formed from the fp64 sums.  Same ulp bound as the centred case; bit-equal share >= torch's bf16 group_norm on the
    same input - 0.01.  Measured on MI355X with the variance formed in fp32 (before the fix): bit-equal 0.932 / 0.927 / 0.886 / 0.927
    against torch's 0.991 / 0.992 / 0.993 / 0.995, every element within 1 ulp - the share failed, as the CPU emulation of that
    arithmetic predicts to the digit (tests/test_vae_refs_cpu.py); after it 0.998 / 0.995 / 0.996 / 0.997."""
    x, gm, bt = R.gn_inputs(C, H, W, "offset")
    ref = R.gn_ref(x, gm, bt, False)
    t = R.ulp_check(R.gn_torch_bf16(x, gm, bt, False), ref, max_ulp=1, frac_exact=0.0)
    got = _gn_run(pkg, gpu, x, gm, bt, False)
    r = R.ulp_check(got[:, 1:1 + H, 1:1 + W].permute(3, 0, 1, 2), ref, max_ulp=1, frac_exact=t["exact"] - 0.01)
    say(f"groupnorm offset frames C{C} {H}x{W}", r, f"  torch bf16: exact {t['exact']:.5f} worst {t['worst_ulp']:.2f} ulp")
    assert r["ok"], R.fmt(r)


@pytest.mark.parametrize("kind", ["centred", "offset"])
@pytest.mark.parametrize("C,cuts", [(128, (0, 3, 10)), (512, (0, 1, 6, 10)), (192, (0, 4, 5, 10))])
def test_groupnorm_row_bands_equal_the_whole_frame(pkg, gpu, C, cuts, kind):
    """drn_groupnorm_stats + drn_groupnorm_apply on unequal row bands (each its own halo-1 buffer), partial sums concatenated,
    applied with the whole frame's count: stitched together == drn_groupnorm_silu on the whole frame, bit for bit."""
    V = pkg.native_vae
    H, W = 10, 13
    x, gm, bt = R.gn_inputs(C, H, W, kind)
    gmd, btd = gm.to(gpu), bt.to(gpu)
    whole = V.groupnorm_silu(to_cl(V, x, gpu), gmd, btd, True).interior().cpu()
    bands = [to_cl(V, x[:, :, a:b].contiguous(), gpu) for a, b in zip(cuts[:-1], cuts[1:])]
    part = torch.cat([V.groupnorm_stats(bd) for bd in bands], 1).contiguous()
    assert part.shape == (4, 64 * len(bands), 2)
    out = torch.cat([V.groupnorm_apply(bd, part, float(H) * W * C, gmd, btd, True).interior().cpu() for bd in bands], 1)
    same = (out == whole).float().mean().item()
    say(f"groupnorm bands C{C} {kind} cuts {cuts}", extra=f"share equal to the whole frame {same:.6f}")
    assert torch.equal(out, whole)


# ------------------------------------------------------------------------------------------------ row softmax
@pytest.mark.parametrize("scale", [1.0, 512 ** -0.5])
@pytest.mark.parametrize("n,extra", R.SOFTMAX_CASES)
def test_softmax_rows_relative_bound(pkg, gpu, n, extra, scale):
    """Every probability within 1 bf16 ulp of the fp64 softmax rounded to bf16 (+ 2^-24): the small ones count."""
    V = pkg.native_vae
    full, s = R.softmax_inputs(n, extra, scale)
    ldp = (n + 63) // 64 * 64 + (64 if extra else 0)
    sg = full.to(gpu)[:, :n]
    assert sg.stride(0) == n + extra
    p = V.softmax_rows(sg, n, ldp, scale).cpu()
    assert p.shape == (R.SOFTMAX_ROWS, ldp) and (p[:, n:] == 0).all()
    ref = R.softmax_ref(s, scale)
    r = R.softmax_check(p[:, :n].contiguous(), ref)
    say(f"softmax n={n} ld={n + extra} ldp={ldp} scale={scale:.4f}", r)
    assert r["ok"], R.fmt(r)
    assert (p[:, :n].float().sum(-1) - 1).abs().max().item() < 2e-2
    assert torch.equal(p[6, :n], torch.full((n,), 1.0 / n, dtype=torch.float64).to(BF)), "constant row"


# ------------------------------------------------------------------------------------------------ temporal attention
@pytest.mark.parametrize("T,C,P", R.TATTN_CASES)
def test_temporal_attention_every_variant(pkg, gpu, T, C, P):
    """Every TMAX instantiation with T == TMAX and T < TMAX, C = 128 (16 lanes), 512 (all 64) and 1024 (second loop trip)."""
    V = pkg.native_vae
    q, k, v = R.tattn_inputs(T, C, P)
    scale = C ** -0.5
    o = V.temporal_attention(q.to(gpu), k.to(gpu), v.to(gpu), scale).cpu()
    ref, mag = R.attn_ref(q, k, v, scale, True)
    r = R.attn_check(o, ref, mag)
    say(f"temporal attn T{T} C{C} P{P}", r)
    assert r["ok"], R.fmt(r)
    if T == 1:
        assert torch.equal(o, v)


@pytest.mark.parametrize("T,C", [(5, 512), (16, 1024), (4, 128)])
def test_temporal_attention_is_causal(pkg, gpu, T, C):
    V = pkg.native_vae
    q, k, v = (t.to(gpu) for t in R.tattn_inputs(T, C, 37, seed=7))
    o = V.temporal_attention(q, k, v, C ** -0.5)
    for t in range(T - 1):
        q2, k2, v2 = q.clone(), k.clone(), v.clone()
        for a in (q2, k2, v2):
            a[t + 1:] = (a[t + 1:].float() * -3 + 1).to(BF)
        o2 = V.temporal_attention(q2, k2, v2, C ** -0.5)
        assert torch.equal(o2[:t + 1], o[:t + 1]), f"output frames <= {t} changed with input frames > {t}"
        assert not torch.equal(o2[t + 1:], o[t + 1:])


@pytest.mark.parametrize("T,C", [(8, 512), (16, 128), (3, 1024)])
def test_temporal_attention_one_hot_exact_integers(pkg, gpu, T, C):
    """Query t matches exactly one key j(t) <= t (score 1600 against 0 at scale 1: the other weights underflow to 0), small
    integer V: the output must be V[j(t)] bit for bit, per pixel - catches a slip in the lane / chunk / frame indexing."""
    V = pkg.native_vae
    P = 37
    g = torch.Generator().manual_seed(T)
    j = torch.stack([torch.randint(0, t + 1, (P,), generator=g) for t in range(T)])           # [T, P]
    col = (torch.arange(T).view(T, 1) * 29 + torch.arange(P).view(1, P) * 8 + 3) % C           # key (t, p) lives at this column
    q, k = torch.zeros((T, P, C)), torch.zeros((T, P, C))
    k.scatter_(2, col.unsqueeze(-1), 40.0)
    q.scatter_(2, torch.gather(col, 0, j).unsqueeze(-1), 40.0)
    v = ((torch.arange(T * P * C).reshape(T, P, C) * 7) % 251 - 125).float()
    o = V.temporal_attention(q.to(BF).to(gpu), k.to(BF).to(gpu), v.to(BF).to(gpu), 1.0).cpu()
    want = torch.gather(v, 0, j.unsqueeze(-1).expand(T, P, C)).to(BF)
    assert torch.equal(o, want), f"{(o != want).sum().item()} of {o.numel()} differ"


def test_temporal_attention_refuses_what_it_cannot_run(pkg, gpu):
    V = pkg.native_vae
    for T, C in ((17, 128), (4, 124)):
        x = torch.zeros((T, 3, C), dtype=BF, device=gpu)
        with pytest.raises(RuntimeError, match="drn_temporal_attention failed"):
            V.temporal_attention(x, x, x, 1.0)


# ------------------------------------------------------------------------------------------------ layout moves, resampling
@pytest.mark.parametrize("C,Cs,halo", [(16, 64, 1), (16, 64, 0), (64, 64, 1), (64, 64, 0)])
def test_planar_cl_moves(pkg, gpu, C, Cs, halo):
    """Bit-exact against torch indexing; tail channels and halo of a pre-filled buffer stay untouched; round trip."""
    V = pkg.native_vae
    lib = pkg.native.load_library()
    T, H, W = 3, 5, 7
    x = R.rnd((C, T, H, W), seed=61)
    fill = torch.full((T, H + 2 * halo, W + 2 * halo, Cs), 7.0, dtype=BF)
    buf, xg = fill.to(gpu), x.to(gpu)
    pkg.native._check(lib.drn_planar_to_cl(xg.data_ptr(), buf.data_ptr(), C, T, H, W, Cs, halo, pkg.native._stream()), "drn_planar_to_cl")
    assert torch.equal(buf.cpu(), R.planar_to_cl_ref(x, Cs, halo, fill))
    cl = V.planar_to_cl(xg, Cs, halo)
    assert torch.equal(cl.t.cpu(), R.planar_to_cl_ref(x, Cs, halo, torch.zeros_like(fill)))
    assert torch.equal(V.cl_to_planar(cl, C).cpu(), x)
    assert torch.equal(V.cl_to_planar(V.CL(T, H, W, Cs, halo, gpu, tensor=buf), C).cpu(), x)
    say(f"planar<->cl C{C} Cs{Cs} halo{halo}", extra="bit-exact")


@pytest.mark.parametrize("rows,cols,extra", [(24, 512, 0), (100, 72, 24), (37, 45, 3), (2304, 512, 0)])
def test_transpose_ragged(pkg, gpu, rows, cols, extra):
    V = pkg.native_vae
    big = R.rnd((rows, cols + extra), seed=62).to(gpu)
    x = big[:, :cols]
    ldo = (rows + 63) // 64 * 64
    y = V.transpose(x, ldo).cpu()
    assert torch.equal(y[:, :rows], x.cpu().t()) and (y[:, rows:] == 0).all()
    say(f"transpose {rows}x{cols} ldx{cols + extra}", extra="bit-exact")


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("T", [1, 2, 4, 5])
def test_resample_every_mode(pkg, gpu, T, C):
    V = pkg.native_vae
    x = R.rnd((C, T, 6, 10), seed=63 + T)
    xc = to_cl(V, x, gpu)
    for mode in range(4):
        y = V.resample(xc, mode)
        want = R.resample_ref(x, mode)
        assert torch.equal(y.t.cpu(), stored(want, C, 1)), f"mode {mode}"
    say(f"resample modes 0-3 T{T} C{C}", extra="bit-exact")


@pytest.mark.parametrize("T,H,W", [(1, 8, 4), (5, 4, 4), (1, 16, 24)])
def test_haar_at_one_frame_and_narrow_images(pkg, gpu, T, H, W):
    V = pkg.native_vae
    orc = VO.VaeOracle({}, pkg.synthetic_weights.COSMOS_CV8x8x8, BF)
    x = R.rnd((3, T, H, W), seed=64)
    ref = orc.patch(x[None])[0]
    got = V.haar_patch(x.to(gpu))
    assert torch.equal(got.t.cpu(), stored(ref, 192, 1))
    p = R.rnd((192, (T + 3) // 4, H // 4, W // 4), seed=65)
    back = V.haar_unpatch(to_cl(V, p, gpu)).cpu()
    assert torch.equal(back, orc.unpatch(p[None])[0])
    say(f"haar T{T} {H}x{W}", extra="bit-exact")


# ------------------------------------------------------------------------------------------------ spatial attention chain
@pytest.mark.parametrize("P", R.SPATIAL_ATTN_KEYS)
def test_spatial_attention_chain_as_the_model_runs_it(pkg, gpu, P):
    """scores_f32 -> softmax_rows(scale) -> transpose -> native.gemm(p, vt) (the tile GEMM the model takes at C = 512), key counts
    that are not multiples of 64 included, against fp64 attention with the flash-attention tests' bound."""
    V = pkg.native_vae
    C = 512
    q, k, v = R.spatial_attn_inputs(P, C)
    scale = 1.0 / math.sqrt(C)
    kp = (P + 63) // 64 * 64
    s = V.scores_f32(q.to(gpu), k.to(gpu))
    p = V.softmax_rows(s, P, kp, scale)
    vt = V.transpose(v.to(gpu), kp)
    o = torch.empty((P, C), dtype=BF, device=gpu)
    pkg.native.gemm(p, vt, out=o)
    ref, mag = R.attn_ref(q[:, None], k[:, None], v[:, None], scale, False)
    r = R.attn_check(o.cpu(), ref[:, 0], mag[:, 0])
    say(f"spatial attn chain P{P} C{C}", r)
    assert r["ok"], R.fmt(r)
