"""fp64 references, comparators, input builders and a conv-geometry recorder for the tokenizer kernel tests
(tests/test_vae_kernels_gpu.py on the GPU, tests/test_vae_refs_cpu.py for the comparators themselves).  Nothing here touches
the GPU: inputs are built on the CPU, references are computed in fp64 from the bf16 inputs with the kernels' DOCUMENTED
rounding points and nothing else, and the plain-torch stand-ins (with optional mutations) exist to show that every bound
passes a correct bf16 implementation and fails a subtly wrong one."""
import math
from collections import namedtuple
from contextlib import contextmanager

import torch
import torch.nn.functional as F

BF = torch.bfloat16
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ comparator
def ulp_check(out, ref64, mag=None, max_ulp=1, frac_exact=0.98, atol_rel=2e-3, atol_abs=0.0):
    """out (bf16) against the fp64 reference ROUNDED to bf16: |out - ref16| <= max_ulp bf16 ulps of max(|out|, |ref16|, mag)
    + atol_rel * rms(ref) (cancellation near zero) + atol_abs, and a share of at least frac_exact bit-equal elements (the
    `ulp_diff_ok` of tests/test_kernels_gpu.py).  Returns a dict with the figures: ok, bad, worst_ulp, exact, rel_l2."""
    assert out.dtype == BF and out.shape == ref64.shape, (out.dtype, out.shape, ref64.shape)
    out = out.cpu()
    r16 = ref64.to(BF)
    o, r = out.double(), r16.double()
    ulp = torch.maximum(o.abs(), r.abs())
    if mag is not None:
        ulp = torch.maximum(ulp, mag.double())
    ulp = ulp * 2.0 ** -7
    atol = atol_rel * ref64.double().pow(2).mean().sqrt().item() + atol_abs
    diff = (o - r).abs()
    bad = int((diff > max_ulp * ulp + atol).sum().item())
    worst = ((diff - atol).clamp_min(0) / ulp.clamp_min(1e-300)).max().item() if diff.numel() else 0.0
    exact = (out == r16).double().mean().item() if diff.numel() else 1.0
    rel = ((out.double() - ref64.double()).norm() / ref64.double().norm().clamp_min(1e-300)).item()
    return {"ok": bad == 0 and exact >= frac_exact, "bad": bad, "worst_ulp": worst, "exact": exact, "rel_l2": rel}


def fmt(res):
    return f"worst {res['worst_ulp']:.2f} ulp  exact {res['exact']:.5f}  rel-L2 {res['rel_l2']:.3e}  bad {res['bad']}"


def rnd(shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF)


def rint(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g)


# ------------------------------------------------------------------------------------------------ convolution
# One launch of native_vae.conv3d without its sizes: cin / cs are the STORED channel counts of input / output, cout the live
# output channels, res one of None, "fresh" (its own buffer), "input" (aliases the input), "output" (in place: aliases the output).
ConvGeom = namedtuple("ConvGeom", "cin cout cs k stride pad t_off in_halo out_halo res")


def geom(cin, cout, k, stride=(1, 1, 1), pad=0, t_off=None, in_halo=1, out_halo=1, res=None, cs=None):
    if t_off is None:
        t_off = (k[0] - 1) + (1 - stride[0])
    return ConvGeom(cin, cout, cs or cout, tuple(k), tuple(stride), pad, t_off, in_halo, out_halo, res)


def conv_out_dims(g, T, H, W):
    """Output dims as the tokenizer asks for them: the strided spatial conv covers the (0,1,0,1)-padded image."""
    kT, kH, kW = g.k
    sT, sH, sW = g.stride
    To = (T + g.t_off - kT) // sT + 1 if (kT > 1 or sT > 1) else T
    if sH == 2:
        return To, H // 2, W // 2
    return To, (H + 2 * g.pad - kH) // sH + 1, (W + 2 * g.pad - kW) // sW + 1


def conv_sizes(g):
    """Input sizes (T, H, W) that give every geometry: M < 128 with T = 1; M an exact multiple of 128 and 256; a ragged
    last tile with a Wo that does not divide the tile (rows wrap inside a tile) and enough frames that the causal clamp acts
    on output frames 0 and 1 and not later."""
    out = []
    for To, Ho, Wo in ((1, 6, 10), (4, 8, 16), (5, 7, 11)):
        T = 2 * To - 1 if g.stride[0] == 2 else To
        H, W = (2 * Ho, 2 * Wo) if g.stride[1] == 2 else (Ho + (g.k[1] - 1) - 2 * g.pad, Wo + (g.k[2] - 1) - 2 * g.pad)
        assert conv_out_dims(g, T, H, W) == (To, Ho, Wo), (g, T, H, W)
        out.append((T, H, W))
    return out


def conv_inputs(g, T, H, W, integer, seed=0, cin_live=None):
    """x [cin, T, H, W], w [cout, cin, kT, kH, kW], bias [cout], res [cout, To, Ho, Wo] or None (all bf16, CPU).
    integer: activations in [-8, 8], weights in [-4, 4] (random in [-3, 3] plus a row / tap / channel dependent offset so no
    two taps, channels or output channels look alike), integer bias and residual: every partial sum is an integer < 2^24."""
    To, Ho, Wo = conv_out_dims(g, T, H, W)
    kT, kH, kW = g.k
    taps = kT * kH * kW
    if integer:
        assert 8 * 4 * taps * g.cin + 16 + 64 < 2 ** 24
        x = rint((g.cin, T, H, W), -8, 8, seed + 1)
        w = rint((g.cout, g.cin, kT, kH, kW), -3, 3, seed + 2)
        n = torch.arange(g.cout).view(-1, 1, 1)
        c = torch.arange(g.cin).view(1, -1, 1)
        tp = torch.arange(taps).view(1, 1, -1)
        w = w + ((n + 2 * tp + 3 * c + (n * tp) % 5) % 3 - 1).view(g.cout, g.cin, kT, kH, kW)
        b = rint((g.cout,), -16, 16, seed + 3)
        r = rint((g.cout, To, Ho, Wo), -64, 64, seed + 4)
        x, w, b, r = x.to(BF), w.to(BF), b.to(BF), r.to(BF)
    else:
        x = rnd((g.cin, T, H, W), 1.0, seed + 1)
        w = rnd((g.cout, g.cin, kT, kH, kW), 1.0 / math.sqrt(g.cin * taps), seed + 2)
        b = rnd((g.cout,), 0.1, seed + 3)
        r = rnd((g.cout, To, Ho, Wo), 1.0, seed + 4)
    if cin_live is not None:                       # a 16-live-of-64 input: zero channel tail, zero K padding of the weights
        x[cin_live:] = 0
        w[:, cin_live:] = 0
    if g.res is None:
        r = None
    elif g.res == "input":                         # the up-sampler's  x + conv(x): same dims, same channels
        assert (g.cin, T, H, W) == (g.cout, To, Ho, Wo)
        r = x.clone()
    return x, w, b, r


def conv_padded_input(g, x, T, H, W, dt, clamp=True, t_off=None):
    """The causal / spatial padding as the layer defines it (CosmosCausalConv3d): frame 0 repeated t_off times in front, `pad`
    zeros around the image, and zeros right / below as far as the strided conv reaches."""
    To, Ho, Wo = conv_out_dims(g, T, H, W)
    t_off = g.t_off if t_off is None else t_off
    x = x.to(dt)[None]
    if t_off:
        front = x[:, :, :1] if clamp else torch.zeros_like(x[:, :, :1])
        x = torch.cat([front] * t_off + [x], 2)
    need_h = (Ho - 1) * g.stride[1] + g.k[1] - (H + g.pad)
    need_w = (Wo - 1) * g.stride[2] + g.k[2] - (W + g.pad)
    return F.pad(x, (g.pad, max(need_w, 0), g.pad, max(need_h, 0), 0, 0))


def conv_ref(g, x, w, b, res, T, H, W):
    """fp64: bf16(conv64 + bias), then bf16(. + residual) (the epilogue of csrc/conv_igemm.hip).  Returns (ref64 of the last
    rounding's argument [cout, To, Ho, Wo], mag): mag = max(|conv|, |res|) when there is a residual (the add may cancel)."""
    To, Ho, Wo = conv_out_dims(g, T, H, W)
    y = F.conv3d(conv_padded_input(g, x, T, H, W, F64), w.double(), b.double(), stride=g.stride)[0][:, :To, :Ho, :Wo]
    assert y.shape == (g.cout, To, Ho, Wo), (y.shape, g)
    if res is None:
        return y, None
    y16 = y.to(BF).double()
    return y16 + res.double(), torch.maximum(y16.abs(), res.double().abs())


def conv_standin(g, x, w, b, res, T, H, W, mutant=None):
    """Plain torch with the kernel's rounding points: fp32 conv (+ bias) rounded to bf16, then the residual add.  mutant:
    'swap_khkw', 'border_tap' (tap (0,0,0) reads one pixel further left for the last output column only), 'zero_causal'
    (zero frames instead of the causal clamp), 't_off' (one frame too many in front), 'bias_late' (bias after the rounding)."""
    To, Ho, Wo = conv_out_dims(g, T, H, W)
    w32 = w.float()
    if mutant == "swap_khkw":
        assert g.k[1] == g.k[2] > 1
        w32 = w32.transpose(-1, -2).contiguous()
    xp = conv_padded_input(g, x, T, H, W, torch.float32, clamp=mutant != "zero_causal",
                           t_off=g.t_off + 1 if mutant == "t_off" else None)
    bias = None if mutant == "bias_late" else b.float()
    y = F.conv3d(xp, w32, bias, stride=g.stride)[0][:, :To, :Ho, :Wo]
    if mutant == "border_tap":
        w0 = torch.zeros_like(w32)
        w0[:, :, 0, 0, 0] = w32[:, :, 0, 0, 0]
        shifted = torch.roll(xp, 1, dims=-1)
        d = F.conv3d(shifted - xp, w0, None, stride=g.stride)[0][:, :To, :Ho, :Wo]
        y = y.clone()
        y[..., Wo - 1] += d[..., Wo - 1]
    y = y.to(BF)
    if mutant == "bias_late":
        y = (y.float() + b.float().view(-1, 1, 1, 1)).to(BF)
    if res is not None:
        y = (y.float() + res.float()).to(BF)
    return y


def conv_model_cases():
    """The tokenizer's channel counts (random-data cases): (tag, geometry, cin_live)."""
    s3, t3, one = (1, 3, 3), (3, 1, 1), (1, 1, 1)
    return [
        ("conv_in 192->128 (1,3,3)", geom(192, 128, s3, pad=1), None),
        ("shortcut 128->256 1x1x1", geom(128, 256, one), None),
        ("256->256 (1,3,3)", geom(256, 256, s3, pad=1), None),
        ("256->256 (3,1,1) + res", geom(256, 256, t3, res="fresh"), None),
        ("512->512 (1,3,3)", geom(512, 512, s3, pad=1), None),
        ("512->512 (1,3,3) + x (up-sampler)", geom(512, 512, s3, pad=1, res="input"), None),
        ("512->512 (3,1,1)", geom(512, 512, t3), None),
        ("512->512 (3,1,1) + res", geom(512, 512, t3, res="fresh"), None),
        ("512->512 (3,1,1) + x (up-sampler)", geom(512, 512, t3, res="input"), None),
        ("down (1,3,3)/2 128 + res", geom(128, 128, s3, stride=(1, 2, 2), res="fresh"), None),
        ("down (3,1,1)/2 t_off 2 256 + res", geom(256, 256, t3, stride=(2, 1, 1), t_off=2, res="fresh"), None),
        ("conv_out 512->16(64) (1,3,3)", geom(512, 16, s3, pad=1, cs=64), None),
        ("16(64)->16(64) (3,1,1)", geom(64, 16, t3, cs=64), 16),
        ("quant 16(64)->16(64) 1x1x1", geom(64, 16, one, cs=64), 16),
        ("post_quant 16(64)->16(64) in place", geom(64, 16, one, cs=64, res="output"), 16),
        ("decoder.conv_out 256->192 (1,3,3)", geom(256, 192, s3, pad=1), None),
        ("192->192 (3,1,1)", geom(192, 192, t3), None),
        ("to_q 512->512 1x1x1 no out halo", geom(512, 512, one, out_halo=0), None),
        ("to_out 512->512 1x1x1 no in halo + res", geom(512, 512, one, in_halo=0, res="fresh"), None),
    ]


CONV_MODEL_SEED = 50


def conv_model_size(g):
    """Input size of the random-data cases: 1920 output positions (15 tiles of 128, 7.5 of 256), five frames."""
    T = 5 if g.stride[0] == 1 else 9
    return (T, 32, 48) if g.stride[1] == 2 else (T, 16, 24)


def conv_edge_geoms():
    """Hand-written geometries for the exact-integer test, whatever the model happens to record."""
    s3, t3, one, f3 = (1, 3, 3), (3, 1, 1), (1, 1, 1), (3, 3, 3)
    return [
        geom(192, 128, s3, pad=1), geom(512, 512, s3, pad=1, res="fresh"), geom(512, 512, t3, res="input"),
        geom(512, 16, s3, pad=1, cs=64), geom(64, 16, t3, cs=64), geom(64, 16, one, cs=64, res="output"),
        geom(256, 192, s3, pad=1), geom(512, 512, one, out_halo=0), geom(512, 512, one, in_halo=0, res="fresh"),
        geom(128, 128, s3, stride=(1, 2, 2), res="fresh"), geom(128, 128, t3, stride=(2, 1, 1), t_off=2, res="fresh"),
        geom(64, 256, f3, pad=1, res="output"), geom(64, 64, s3, in_halo=1, out_halo=0, pad=0),
    ]


class ConvRecorder:
    """Notes the geometry of every native_vae.conv3d call made while it is active (see `record_convs`)."""

    def __init__(self, names=None):
        self.names = names or {}            # weight data_ptr -> parameter name
        self.geoms = {}                     # ConvGeom -> list of names
        self.seen = set()

    def note(self, x, w, N_out, k, stride, pad, t_off, residual, result):
        kind = None
        if residual is not None:
            kind = "input" if residual is x else ("output" if residual is result else "fresh")
        g = geom(x.C, N_out, k, stride, pad, t_off, x.halo, result.halo, kind, result.C)
        assert (result.T, result.H, result.W) == conv_out_dims(g, x.T, x.H, x.W), (g, (x.T, x.H, x.W), (result.T, result.H, result.W))
        name = self.names.get(w.data_ptr(), "?")
        self.geoms.setdefault(g, []).append(name)
        self.seen.add(name)


@contextmanager
def record_convs(native_vae, names=None):
    rec = ConvRecorder(names)
    orig = native_vae.conv3d

    def conv3d(x, w, bias, N_out, k, stride=(1, 1, 1), pad=0, t_off=None, out=None, residual=None, out_halo=1, out_dims=None,
               out_channels_stored=None):
        y = orig(x, w, bias, N_out, k, stride, pad, t_off, out, residual, out_halo, out_dims, out_channels_stored)
        rec.note(x, w, N_out, k, stride, pad, t_off, residual, y)
        return y

    native_vae.conv3d = conv3d
    try:
        yield rec
    finally:
        native_vae.conv3d = orig


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_CASES = [(C, H, W) for C, ws in ((128, (5, 16, 37)), (256, (3, 8, 21)), (512, (2, 4, 11)), (192, (7,)), (320, (7,)))
            for H, W in [(6, w) for w in ws] + [(1, ws[-1])]]       # W below / equal to / not a multiple of 256 / (C/8); H = 1


GN_OFFSET_CASES = [(128, 9, 11), (256, 6, 21), (512, 6, 11), (192, 9, 11)]


def gn_inputs(C, H, W, kind="centred", seed=0):
    """x [C, 4, H, W] bf16 with a different mean and scale per frame, gamma, beta [C].  kind 'offset': frames with a mean of
    about 125, 125, 250 and 32 times their spread (64 + 0.5 z, 256 + 2 z, 1000 + 4 z, -16 + 0.5 z, rounded to bf16)."""
    z = torch.randn((C, 4, H, W), generator=torch.Generator().manual_seed(1000 + seed))
    if kind == "centred":
        mean, scale = (0.0, 0.5, -1.0, 2.0), (1.0, 2.0, 0.5, 3.0)
    else:
        mean, scale = (64.0, 256.0, 1000.0, -16.0), (0.5, 2.0, 4.0, 0.5)
    x = (z * torch.tensor(scale).view(1, 4, 1, 1) + torch.tensor(mean).view(1, 4, 1, 1)).to(BF)
    return x, (1 + 0.1 * rnd((C,), seed=seed + 14).float()).to(BF), rnd((C,), 0.2, seed=seed + 15)


def silu64(x):
    return x * torch.sigmoid(x)


def gn_ref(x, gamma, beta, silu, eps=1e-6):
    """fp64 per-frame GroupNorm (one group): bf16(gn64), then (if silu) silu64 of that rounded value.  Returns the fp64 argument
    of the LAST rounding, [C, T, H, W]."""
    x = x.double()
    mean = x.mean(dim=(0, 2, 3), keepdim=True)
    var = (x - mean).pow(2).mean(dim=(0, 2, 3), keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double().view(-1, 1, 1, 1) + beta.double().view(-1, 1, 1, 1)
    return silu64(y.to(BF).double()) if silu else y


def gn_torch_bf16(x, gamma, beta, silu, eps=1e-6):
    """torch's own bf16 group_norm (per frame) - the yardstick for what a correct bf16 implementation reaches."""
    y = F.group_norm(x.permute(1, 0, 2, 3), 1, gamma, beta, eps).permute(1, 0, 2, 3)
    return F.silu(y) if silu else y


def gn_standin(x, gamma, beta, silu, eps=1e-6, mutant=None):
    """The kernel's arithmetic in torch: fp64 sums, fp32 mean / rstd, fp32 normalise, bf16, fp32 SiLU.  mutant 'fp32_var': the
    sums are cast to fp32 BEFORE var = q / n - mean^2 (the kernel before the fix); 'frame0': frame 0's statistics for all."""
    xd = x.double()
    n = float(x.shape[0] * x.shape[2] * x.shape[3])
    s, q = xd.sum(dim=(0, 2, 3), keepdim=True), xd.pow(2).sum(dim=(0, 2, 3), keepdim=True)
    if mutant == "frame0":
        s, q = s[:, :1].expand_as(s), q[:, :1].expand_as(q)
    if mutant == "fp32_var":
        s32, q32 = s.float(), q.float()
        mean = s32 / n
        var = (q32 / n - mean * mean).clamp_min(0)
        rstd = 1.0 / torch.sqrt(var + eps)
    else:
        meand = s / n
        var = (q / n - meand * meand).clamp_min(0)
        mean, rstd = meand.float(), (1.0 / torch.sqrt(var + eps)).float()
    y = (((x.float() - mean) * rstd) * gamma.float().view(-1, 1, 1, 1) + beta.float().view(-1, 1, 1, 1)).to(BF)
    return (y.float() * torch.sigmoid(y.float())).to(BF) if silu else y


# ------------------------------------------------------------------------------------------------ row softmax
# (n, ld - n): every kernel variant (registers with 4 / 9 / 16 vectors per thread, three-pass) at and just past its boundary
SOFTMAX_CASES = [(37, 0), (100, 0), (100, 28), (4096, 0), (4096, 64), (4100, 0), (4098, 62), (9216, 0), (9216, 64), (9220, 4),
                 (16384, 0), (16384, 64), (16388, 0), (16388, 60)]
SOFTMAX_ROWS = 8


def softmax_inputs(n, extra, scale):
    """fp32 scores [8, n] as a view of an [8, n + extra] matrix; softmax(scale * s) sees N(0, 3) rows, then special rows:
    4 one dominant score in the first column, 5 in the last, 6 constant, 7 one score of -1e4 (after scaling)."""
    g = torch.Generator().manual_seed(7 * n + extra)
    full = torch.randn((SOFTMAX_ROWS, n + extra), generator=g) * 3.0
    s = full[:, :n]
    s[4, 0] = 40.0
    s[5, n - 1] = 40.0
    s[6] = 1.25
    s[7, n // 2] = -1e4
    full /= scale
    return full, s


def softmax_ref(s, scale):
    return torch.softmax(s.double() * float(torch.tensor(scale, dtype=torch.float32)), -1)


def softmax_standin(s, scale, mutant=None):
    p = torch.softmax(s.float() * scale, -1)
    if mutant == "small_3pct":
        p = torch.where(p < 1e-3, p * 1.03, p)
    return p.to(BF)


def softmax_check(out, ref64):
    """Every probability within 1 bf16 ulp of the reference rounded to bf16 plus 2^-24 absolute: a RELATIVE bound, the small
    probabilities count as much as the large ones."""
    return ulp_check(out, ref64, max_ulp=1, frac_exact=0.0, atol_rel=0.0, atol_abs=2.0 ** -24)


# ------------------------------------------------------------------------------------------------ temporal attention
TATTN_CASES = [(1, 512, 37), (2, 128, 3), (2, 512, 256), (3, 512, 37), (3, 128, 1), (4, 1024, 3), (4, 128, 256), (5, 512, 37),
               (5, 1024, 1), (8, 512, 256), (8, 128, 1), (9, 512, 3), (9, 1024, 37), (16, 512, 37), (16, 128, 256), (16, 1024, 3)]
ATTN_REL_L2 = 3.6e-3          # tests/test_kernels_gpu.py: the flash-attention bound


def tattn_inputs(T, C, P, seed=0):
    return tuple(rnd((T, P, C), seed=100 * T + seed + i) for i in range(3))


def attn_ref(q, k, v, scale, causal):
    """q [Sq, B, C], k, v [Sk, B, C] (B independent problems: the pixels of the temporal attention, 1 for the spatial one):
    fp64 softmax(scale q k^T) v and mag = sqrt(sum p^2 v^2), the size of the terms the output is summed from."""
    qd, kd, vd = (t.double().permute(1, 0, 2) for t in (q, k, v))
    s = qd @ kd.transpose(1, 2) * scale
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(s.shape[-2:], dtype=torch.bool)), float("-inf"))
    p = torch.softmax(s, -1)
    return (p @ vd).permute(1, 0, 2), ((p * p) @ (vd * vd)).sqrt().permute(1, 0, 2)


SPATIAL_ATTN_KEYS = (24, 100, 2304)          # key counts of the spatial-attention chain (two are not multiples of 64), C = 512


def spatial_attn_inputs(P, C=512):
    return tuple(rnd((P, C), seed=70 + i) for i in range(3))


def tattn_standin(q, k, v, scale, p_bf16=True, mutant=None, causal=True):
    """fp32 scores, softmax, P rounded to bf16 (the kernel's design) or left in fp32, fp32 P.V, bf16 out.  mutant 'no_mask'."""
    qf, kf, vf = (t.float().permute(1, 0, 2) for t in (q, k, v))
    s = qf @ kf.transpose(1, 2) * scale
    if causal and mutant != "no_mask":
        s = s.masked_fill(~torch.tril(torch.ones(s.shape[-2:], dtype=torch.bool)), float("-inf"))
    p = torch.softmax(s, -1)
    if p_bf16:
        p = p.to(BF).float()
    return (p @ vf).permute(1, 0, 2).to(BF)


def attn_check(out, ref64, mag):
    """The bound of the flash-attention tests (`_attn_check`): <= 2 bf16 ulp of max(|o|, |ref|, sqrt(sum p^2 v^2)), at least half
    bit-equal, rel-L2 <= ATTN_REL_L2."""
    res = ulp_check(out, ref64, mag=mag, max_ulp=2, frac_exact=0.5, atol_rel=0.0)
    res["ok"] = res["ok"] and res["rel_l2"] <= ATTN_REL_L2
    return res


# ------------------------------------------------------------------------------------------------ layout moves, resampling
def planar_to_cl_ref(x, Cs, halo, fill):
    """[C, T, H, W] -> stored [T, H + 2 halo, W + 2 halo, Cs]; tail channels and halo keep `fill` (what the buffer held)."""
    C, T, H, W = x.shape
    out = fill.clone()
    assert out.shape == (T, H + 2 * halo, W + 2 * halo, Cs)
    out[:, halo:halo + H, halo:halo + W, :C] = x.permute(1, 2, 3, 0)
    return out


def planar_to_cl_standin(x, Cs, halo, fill, mutant=None):
    out = planar_to_cl_ref(x, Cs, halo, fill)
    if mutant == "tail" and Cs > x.shape[0]:
        H, W = x.shape[2:]
        out[:, halo:halo + H, halo:halo + W, x.shape[0]:] = 0
    return out


def resample_ref(x, mode):
    """x [C, T, H, W] bf16 -> bf16, fp64 arithmetic (the means of 2 or 4 bf16 values are exact in fp64)."""
    C, T, H, W = x.shape
    xd = x.double()
    if mode == 0:           # 2 x 2 mean of the (0,1,0,1)-padded image
        return ((xd[:, :, 0::2, 0::2] + xd[:, :, 0::2, 1::2] + xd[:, :, 1::2, 0::2] + xd[:, :, 1::2, 1::2]) * 0.25).to(BF)
    if mode == 1:           # 2-frame mean of [x0, x0, x1, ...]
        xx = torch.cat([xd[:, :1], xd], 1)
        if xx.shape[1] % 2:
            xx = torch.cat([xx, xx[:, -1:]], 1)
        return ((xx[:, 0::2] + xx[:, 1::2]) * 0.5)[:, :(T + 1) // 2].to(BF)
    if mode == 2:           # nearest x 2 in time minus the first frame
        return x if T == 1 else x.repeat_interleave(2, dim=1)[:, 1:]
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
