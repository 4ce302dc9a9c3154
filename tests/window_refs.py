"""References, input builders and wrong stand-ins for the long-clip window join (drn_postprocess_window_u8, windows.py).

Everything here is torch on the CPU.  `blend_postprocess` restates the kernel's contract with eager fp32 torch ops - one rounded
op per step, `a + w * (b - a)`, `.to(bfloat16)` - followed by the pipeline oracle's `postprocess`.  The `variant`s are WRONG
kernels; tests/test_windows_cpu.py shows on the very tensors the GPU test launches that each of them changes at least one output
byte, so `torch.equal` against the reference can tell them from a right kernel.
"""
import torch

from oracle import dit_oracle as O

BF = torch.bfloat16
TW = 9                                        # window length of the kernel cases
SHAPES = [(8, 8), (5, 7), (3, 11), (8, 12)]   # H x W: 8-pixel groups; one-pixel path (35, 33 pixels); 12 groups per frame
OVERLAPS = [0, 1, 2, 4]
VARIANTS = ["fma", "fma_sub_rounded", "reversed", "early", "late", "head", "after_normal", "j_over_O"]


def ramp_table(pkg, overlap):
    return torch.from_numpy(pkg.windows.ramp_weights(overlap))


# ----------------------------------------------------------------------------------------------- the pieces of O.postprocess
def _normal_blend(video):
    norm = torch.norm(video, dim=1, p=2, keepdim=True)
    vn = video / norm.clamp(min=1e-12)
    blend = torch.clip((norm - 0.2) / (0.4 - 0.2), 0, 1)
    return vn * blend + video * (1 - blend)


def _blend(a, b, w, variant):
    """a, b fp32 [B,3,O,H,W], w fp32 [O] -> bf16."""
    w = w.view(1, 1, -1, 1, 1)
    if variant == "fma":                      # contracted: the whole expression in fp64, rounded once to fp32
        return (a.double() + w.double() * (b.double() - a.double())).float().to(BF)
    if variant == "fma_sub_rounded":          # what v_fma_f32 computes: the fp32 difference, then one rounding of w * d + a
        return (a.double() + w.double() * (b - a).double()).float().to(BF)
    return (a + w * (b - a)).to(BF)


def blend_postprocess(video, prev_tail, ramp_w, ramp_at, write_lo, write_hi, normalize_normal, variant=None):
    """video bf16 [B,3,Tw,H,W], prev_tail bf16 [B,3,O,H,W] or None, ramp_w fp32 [O] or None -> uint8 [B, write_hi - write_lo, H, W, 3].
    variant None: the contract.  Otherwise one of VARIANTS (a wrong kernel)."""
    v = video.clone()
    if prev_tail is not None and prev_tail.shape[2] > 0:
        n = prev_tail.shape[2]
        w, at, a = ramp_w, ramp_at, prev_tail
        if variant == "reversed":
            w = ramp_w.flip(0)
        elif variant == "j_over_O":
            w = (torch.arange(n, dtype=torch.float64) / n).float()
        elif variant == "early":
            at = ramp_at - 1
        elif variant == "late":
            at = ramp_at + 1
        elif variant == "head":
            a = video[:, :, :n]
        lo, hi = max(at, 0), min(at + n, video.shape[2])          # a shifted ramp is cut at the window's ends
        a, w = a[:, :, lo - at:hi - at], w[lo - at:hi - at]
        b = video[:, :, lo:hi]
        if variant == "after_normal" and normalize_normal:
            out = torch.cat([_normal_blend(video[:, :, :lo]), _blend(_normal_blend(a).float(), _normal_blend(b).float(), w, None),
                             _normal_blend(video[:, :, hi:])], 2)
            return O.postprocess(out[:, :, write_lo:write_hi], False)
        v[:, :, lo:hi] = _blend(a.float(), b.float(), w, variant)
    return O.postprocess(v[:, :, write_lo:write_hi], normalize_normal)


# ----------------------------------------------------------------------------------------------- inputs of the GPU kernel test
def case_inputs(B, H, W, overlap):
    """The window and the carry of one small kernel case: seeded N(0, 0.8) values as bf16 (most of them inside the clamp, norms on
    both sides of the normal blend's knees), the same for every ramp position and write range."""
    g = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * W + overlap)
    video = (torch.randn((B, 3, TW, H, W), generator=g) * 0.8).to(BF)
    prev = (torch.randn((B, 3, overlap, H, W), generator=g) * 0.8).to(BF) if overlap else None
    return video, prev


def case_geometries(overlap):
    """(ramp_at, write_lo, write_hi) of the small cases: the ramp at the window's head, inside it and at its end; written as a
    middle window (up to the carry), as the last window (to the end), and from frame 0 with the ramp inside the written range."""
    geos = set()
    for ramp_at in (0, 3, TW - overlap):
        for lo, hi in ((ramp_at, TW - overlap), (ramp_at, TW), (0, TW)):
            if 0 <= lo < hi <= TW:                    # (a middle window whose ramp sits at the end would write nothing)
                geos.add((ramp_at, lo, hi))
    return sorted(geos)


def bf16_values(limit=4.0):
    """Every finite bf16 value in [-limit, limit], both zeros included."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF)
    keep = torch.isfinite(v.float()) & (v.float().abs() <= limit)
    return v[keep]


GRID_HW = (128, 128)
GRID_OVERLAPS = [1, 2, 4, 8]


def value_grid(overlap):
    """The value-grid case of one ramp table: a 128 x 128 window (49 152 values per frame, 16-byte aligned planes).  Every ramp
    frame pairs EVERY finite bf16 value in [-4, 4] (as `a`, the carry; +/-0, the clamp edges +/-1 and the normal blend's knees 0.2 /
    0.4 among them) with a seeded draw from the same set (as `b`, the window), and fills the remaining 16 126 values with pairs of
    comparable size, 2^-6 <= |a|, |b| <= 2: there `a + w * (b - a)` of two 8-bit significands and w = fp32(k / n) lands on or
    next to a bf16 tie often enough for a single fused rounding to show (two values of wildly different size never do; w = 1/2, the
    whole O = 1 table, multiplies exactly and cannot).  Pairs are shuffled over the frame, afresh per ramp frame.  ramp_at = 0."""
    H, W = GRID_HW
    vals = bf16_values()
    near = vals[(vals.float().abs() >= 2.0 ** -6) & (vals.float().abs() <= 2.0)]
    n, nv = 3 * H * W, vals.numel()
    g = torch.Generator().manual_seed(7700 + overlap)

    def draw(src, k):
        return src[torch.randint(0, src.numel(), (k,), generator=g)]
    prev = torch.empty((overlap, n), dtype=BF)
    video = draw(vals, TW * n).view(TW, n).clone()
    for j in range(overlap):
        perm = torch.randperm(n, generator=g)
        prev[j] = torch.cat([vals, draw(near, n - nv)])[perm]
        video[j] = torch.cat([draw(vals, nv), draw(near, n - nv)])[perm]
    to5 = lambda t: t.view(t.shape[0], 3, H, W).permute(1, 0, 2, 3).unsqueeze(0).contiguous()   # noqa: E731
    return to5(video), to5(prev)
