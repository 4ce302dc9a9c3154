"""MXFP8 producers that write their result quantised (no quantise launch), host side - no GPU needed:
the new symbols, the refusals every new entry makes before it launches anything, and the teeth of the comparator the GPU tests
use.  The one rule (include/drn.h): a fused producer rounds to bf16 where its twin rounds and quantises THAT value, so its output
must equal drn_mx_quant_bf16(twin's output) bit for bit.  The input generators below are the ones tests/test_mxfp8_fused_gpu.py
feeds the kernels; here torch stand-ins of the three producers show that on these inputs the three plausible mistakes
(quantising the fp32 value, the amax over the wrong 32 columns, forgetting the significand > 1.75 bump) change bytes, and that
the inputs reach an all-zero block, the bump branch and >= 16 binades of block exponents."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import mx_emul as MX
from conftest import ROOT

BF = torch.bfloat16
NEW = ("drn_mx_quant_calls", "drn_gemm_mxfp8_gelu_mx", "drn_ln_modulate_mx", "drn_splitk_gate_res_ln_modulate_mx",
       "drn_attention_bf16_mx", "drn_attention_splitkv_bf16_mx", "drn_attention_mx_available", "drn_dit_forward_mx_u_bytes")


# ------------------------------------------------------------------------------------------------ input generators (CPU tensors)
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def block_gains(nblocks, lo, hi, seed):
    """One power of two per 32-column block, exponents spread evenly over [lo, hi] and shuffled; block 1 gets gain 0."""
    g = _gen(seed)
    e = torch.linspace(lo, hi, nblocks).round()[torch.randperm(nblocks, generator=g)]
    gain = torch.exp2(e)
    gain[1 % nblocks] = 0.0
    return gain


def ln_inputs(rows, D, clips, seed=0):
    """x [rows, D], add_vec / shift / scale [clips, D] bf16.  bf16(1 + scale) is a power of two per 32-column block (2^-10 .. 2^10)
    and exactly 0 in block 1 (scale = -1, shift = 0 there: an all-zero output block); shift follows the gain of its block."""
    g = _gen(seed)
    x = (torch.randn((rows, D), generator=g) * 1.5 + 0.25).to(BF)
    add = (torch.randn((clips, D), generator=g) * 0.5).to(BF)
    nb = D // 32
    gain = torch.stack([block_gains(nb, -10, 10, seed + 1 + c) for c in range(clips)])            # [clips, nb]
    scale = (gain - 1.0).repeat_interleave(32, dim=1).to(BF)
    shift = (torch.randn((clips, D), generator=g) * 0.25 * gain.repeat_interleave(32, dim=1)).to(BF)
    return x, add, shift, scale


def ln_standin(x, add, shift, scale, rows_per_batch, eps=1e-6):
    """fp32 value in front of the last bf16 rounding of drn_ln_modulate (statistics in torch's own order: a stand-in, not the
    kernel's summation tree) -> [rows, D] fp32."""
    rows, D = x.shape
    b = torch.arange(rows) // rows_per_batch
    xv = x.float()
    if add is not None:
        xv = (xv + add.float()[b]).to(BF).float()
    mean = xv.mean(-1, keepdim=True)
    var = ((xv - mean) ** 2).mean(-1, keepdim=True)
    n = ((xv - mean) / torch.sqrt(var + eps)).to(BF).float()
    s1 = (1.0 + scale.float()[b]).to(BF).float()
    return (n * s1).to(BF).float() + shift.float()[b]


def attn_inputs(batch, S, heads, seed=0):
    """q, k, v [batch, S, heads * 128] bf16.  The columns of v carry one power of two per 32-column block (2^-10 .. 2^10, block 1
    zero: an all-zero output block); q . k is sharp enough that the softmax is not uniform."""
    g = _gen(seed)
    HD = heads * 128
    q = torch.randn((batch, S, HD), generator=g).to(BF)
    k = torch.randn((batch, S, HD), generator=g).to(BF)
    gain = block_gains(HD // 32, -10, 10, seed + 1).repeat_interleave(32)
    v = (torch.randn((batch, S, HD), generator=g) * gain).to(BF)
    return q, k, v


def attn_standin(q, k, v, heads):
    """fp32 softmax attention -> [batch * S, heads * 128] fp32 (the value the kernel rounds to bf16)."""
    B, S, HD = q.shape
    sh = lambda t: t.float().view(B, -1, heads, 128).permute(0, 2, 1, 3)
    o = F.scaled_dot_product_attention(sh(q), sh(k), sh(v))
    return o.permute(0, 2, 1, 3).reshape(B * S, HD)


def gelu_inputs(M, N, K, seed=0):
    """a [M, K], w [N, K] bf16; the rows of w (output columns) carry one power of two per block of 32 (2^-14 .. 2^3 around the
    K^-1/2 normalisation; block 1 zero: an all-zero output block)."""
    g = _gen(seed)
    a = torch.randn((M, K), generator=g).to(BF)
    gain = block_gains(N // 32, -14, 3, seed + 1).repeat_interleave(32).view(N, 1)
    w = (torch.randn((N, K), generator=g) * (K ** -0.5) * gain).to(BF)
    return a, w


def gelu_standin(a, w):
    """fp32 GELU of the bf16-rounded product of the MXFP8 quantise -> dequantise operands -> [M, N] fp32."""
    lin = F.linear(MX.qdq(a).float(), MX.qdq(w).float())
    return F.gelu(lin.to(BF).float())


# ------------------------------------------------------------------------------------------------ the comparator and its teeth
def coverage(y):
    """(all-zero blocks, blocks on the significand > 1.75 branch, binades spanned by the non-zero blocks) of a bf16 result [rows, K]."""
    rows, K = y.shape
    amax = y.float().abs().view(rows, K // 32, 32).amax(-1)
    mant, ex = torch.frexp(amax)
    nz = amax > 0
    bump = nz & (mant * 2 > 1.75)
    span = int(ex[nz].max() - ex[nz].min()) + 1 if nz.any() else 0
    return int((~nz).sum()), int(bump.sum()), span


def assert_covers(y, what):
    zero, bump, span = coverage(y)
    assert zero >= 1, (what, "no all-zero block")
    assert bump >= 1, (what, "no block on the bump branch")
    assert span >= 16, (what, f"block exponents span {span} binades")


def _quant_with_exponents(x, e):
    rows, K = x.shape
    xs = x.float().view(rows, K // 32, 32) * MX.pow2(-e).unsqueeze(-1)
    return xs.view(rows, K).to(torch.float8_e4m3fn), (e + 127).to(torch.uint8)


def _same(a, b):
    return torch.equal(a[0].view(torch.uint8), b[0].view(torch.uint8)) and torch.equal(a[1], b[1])


def wrong_fp32_first(r32):
    """quantises the fp32 value, before the bf16 rounding"""
    return MX.quantize(r32)


def wrong_columns(rb):
    """block amax taken 16 columns off"""
    return _quant_with_exponents(rb, MX.block_exponents(torch.roll(rb.float(), 16, dims=1)))


def wrong_no_bump(rb):
    """forgets e + 1 when the significand of amax is above 1.75"""
    rows, K = rb.shape
    amax = rb.float().abs().view(rows, K // 32, 32).amax(-1)
    _, ex = torch.frexp(amax)
    e = torch.where(amax > 0, ex.to(torch.int32) - 9, torch.full_like(ex, -127, dtype=torch.int32)).clamp(-127, 127).to(torch.int32)
    return _quant_with_exponents(rb, e)


def _standins():
    x, add, shift, scale = ln_inputs(300, 1024, 2, seed=11)
    yield "ln", ln_standin(x, add, shift, scale, 150)
    q, k, v = attn_inputs(2, 128, 4, seed=12)
    yield "attention", attn_standin(q, k, v, 4)
    a, w = gelu_inputs(300, 2048, 512, seed=13)
    yield "gelu", gelu_standin(a, w)


def test_comparator_has_teeth_on_the_gpu_tests_inputs():
    for what, r32 in _standins():
        rb = r32.to(BF)
        ref = MX.quantize(rb)
        assert_covers(rb, what)
        assert _same(ref, MX.quantize(rb.clone())), what
        assert not _same(ref, wrong_fp32_first(r32)), (what, "quantising before the bf16 rounding goes unnoticed")
        assert not _same(ref, wrong_columns(rb)), (what, "a 16-column shift of the amax goes unnoticed")
        assert not _same(ref, wrong_no_bump(rb)), (what, "a missing significand > 1.75 bump goes unnoticed")


# ------------------------------------------------------------------------------------------------ symbols and refusals
@pytest.fixture()
def lib(pkg):
    lib = pkg.native.load_library()
    was = lib.drn_gemm_mxfp8_force_small_m(1)
    lib.drn_attention_force_shape16(1)
    yield lib
    lib.drn_gemm_mxfp8_force_small_m(was)
    lib.drn_attention_force_shape16(-1)


def test_new_symbols_declared_bound_and_exported(pkg, lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drn.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in pkg.native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.drn_dit_forward_args_bytes() == ctypes.sizeof(pkg.native.DitForwardArgs)
    for f in ("mx_fused", "UQ", "US", "u_act_bytes"):
        assert hasattr(pkg.native.DitForwardArgs, f), f
    for fn, arg in ((pkg.native.ln_modulate, "out_mx"), (pkg.native.attention, "out_mx"), (pkg.native.gemm_mxfp8, "out_mx")):
        assert arg in fn.__code__.co_varnames, fn.__name__
    assert lib.drn_dit_forward_mx_u_bytes(2, 256, 16384) == 2 * 256 * 16384 * 33 // 32
    assert lib.drn_mx_quant_calls(0) >= 0


P = 1 << 20          # a fake, aligned, never dereferenced device address


def test_ln_entries_refuse_on_the_host(pkg, lib):
    ln, fold = lib.drn_ln_modulate_mx, lib.drn_splitk_gate_res_ln_modulate_mx

    def call(x=P, h=None, hq=P, hs=P, rows=256, D=4096, rpb=256):
        return ln(x, None, P, P, h, hq, hs, rows, D, rpb, 1e-6, None)

    assert call(hq=None) == -1 and call(hs=None) == -1
    assert call(D=4096 + 8) == -1 and call(D=4096 + 16) == -1          # D % 32 (both are fine for the bf16 entry: D % 8)
    assert call(D=8192 + 32) == -1 and call(x=None) == -1 and call(rpb=0) == -1
    assert call(hq=P + 4) == -1                                        # 8-byte stores
    assert call(rows=0) == 0                                           # nothing to do is not an error (as drn_ln_modulate)

    def callf(part=P, hq=P, hs=P, D=4096, splits=2, rows=256):
        return fold(part, splits, P, P, None, P, P, None, hq, hs, rows, D, 256, 1e-6, None)

    assert callf(hq=None) == -1 and callf(hs=None) == -1 and callf(part=None) == -1
    assert callf(D=1024) == -1 and callf(D=4096 + 8) == -1 and callf(splits=0) == -1
    assert callf(rows=0) == 0


def test_attention_entries_refuse_on_the_host(pkg, lib):
    one, split = lib.drn_attention_bf16_mx, lib.drn_attention_splitkv_bf16_mx
    H, S = 4, 256
    HD = H * 128

    def call(oq=P, os_=P, o=None, ldo=HD, bso=S * HD, batch=1, heads=H, Sq=S):
        return one(P, P, P, o, oq, os_, batch, heads, Sq, S, 3 * HD, 3 * HD, 3 * HD, ldo, S * 3 * HD, S * 3 * HD, S * 3 * HD, bso,
                   0.088, None)

    assert call(oq=None) == -1 and call(os_=None) == -1
    assert call(ldo=HD + 8) == -1                  # the MX rows are contiguous: ldo must be heads * 128
    assert call(bso=S * HD + 8) == -1              # clips start on whole rows
    assert call(batch=2, bso=HD) == -1             # ... that do not overlap
    assert call(oq=P + 4) == -1 and call(os_=P + 2) == -1
    assert call(Sq=0) == 0
    assert split(P, P, P, None, P, P, 1, H, S, S, 3 * HD, 3 * HD, 3 * HD, HD, 0, 0, 0, 0, 0.088, 2, None, None) == -1   # workspace
    assert split(P, P, P, None, None, P, 1, H, S, S, 3 * HD, 3 * HD, 3 * HD, HD, 0, 0, 0, 0, 0.088, 2, P, None) == -1
    # the 32x32x16 body has no MX epilogue: refused, and the availability query says so
    assert lib.drn_attention_mx_available() == 1
    lib.drn_attention_force_shape16(0)
    try:
        assert lib.drn_attention_mx_available() == 0 and not pkg.native.attention_mx_available()
        assert call() == -1
        assert split(P, P, P, None, P, P, 1, H, S, S, 3 * HD, 3 * HD, 3 * HD, HD, 0, 0, 0, 0, 0.088, 2, P, None) == -1
    finally:
        lib.drn_attention_force_shape16(1)
    # the bf16 entries still refuse a NULL output
    assert lib.drn_attention_bf16(P, P, P, None, 1, H, S, S, 3 * HD, 3 * HD, 3 * HD, HD, 0, 0, 0, 0, 0.088, None) == -1


def test_gelu_entry_refuses_on_the_host(pkg, lib):
    f = lib.drn_gemm_mxfp8_gelu_mx

    def call(M=256, N=16384, K=4096, cq=P, cs=P, a=P, rpb=0):
        return f(a, P, P, P, cq, cs, M, N, K, rpb, None)

    assert call(cq=None) == -1 and call(cs=None) == -1 and call(a=None) == -1
    assert call(N=16384 + 128) == -1               # N % 256
    assert call(K=4096 + 64) == -1                 # K % 128
    assert call(M=0) == -1 and call(cq=P + 2) == -1
    # a sliced choice: the GELU lives in the reduce launch, no MX form - callers fall back
    assert lib.drn_gemm_mxfp8_splitk_choice(256, 4096, 16384) > 1
    assert call(N=4096, K=16384) == -1
    assert call(M=512, N=4096, K=16384, rpb=256) == -1          # decided from ONE clip's rows
    with pytest.raises(ValueError):
        pkg.native.gemm_mxfp8(pkg.native.MxTensor(torch.empty((256, 16384), dtype=torch.float8_e4m3fn), None),
                              pkg.native.MxTensor(torch.empty((4096, 16384), dtype=torch.float8_e4m3fn), None),
                              epilogue=pkg.native.EPI_GELU, out_mx=True)


def test_forward_refuses_before_any_launch(pkg, lib):
    from test_mxfp8_small_m_cpu import _mx_args
    fwd = lib.drn_dit_forward

    def fused(B=1, S=256, D=4096, hidden=16384):
        a, subs = _mx_args(pkg, lib, B, S, D, hidden)
        a.mx_fused, a.UQ, a.US = 1, P, P
        a.u_act_bytes = lib.drn_dit_forward_mx_u_bytes(B, S, hidden)
        return a, subs

    a, subs = fused()
    a.UQ = None
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused()
    a.US = None
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused()
    a.u_act_bytes -= 1
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused(B=2)
    a.u_act_bytes = lib.drn_dit_forward_mx_u_bytes(1, 256, 16384)           # sized for one clip, two stacked
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused()
    a.mx_fused = 2
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused()
    a.mx_fused = -1
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused()
    a.precision = 0
    assert fwd(ctypes.byref(a), None) == -1
    # the refusals of the unfused forward are still made with the new fields present
    a, subs = fused()
    a.AQ = None
    assert fwd(ctypes.byref(a), None) == -1
    # and so are the per-sub-block ones, which an mx_fused forward used to reach only after its first launches (control first:
    # the unchanged args are not refused; asked only where no GPU is visible, as a GPU would run kernels on the fake addresses)
    import torch
    for kw in ({}, dict(S=16640, D=512, hidden=2048)):
        a, subs = fused(**kw)
        a.attn_ws_bytes = lib.drn_dit_forward_attn_workspace_bytes(1, a.heads, a.S)
        assert torch.cuda.is_available() or fwd(ctypes.byref(a), None) > 0
    a, subs = fused()
    subs[1].kind = 7
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused()
    subs[0].qn = None
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused()
    subs[1].kind, subs[1].ca_index = pkg.native.SUB_CA, 0                      # addvec is NULL in these args
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = fused(S=16640, D=512, hidden=2048)
    a.attn_ws_bytes = lib.drn_dit_forward_attn_workspace_bytes(1, 4, 16640) - 1
    assert a.attn_ws_bytes > 0 and fwd(ctypes.byref(a), None) == -1

