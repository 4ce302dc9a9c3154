"""Every finite bf16 value through the arithmetic that ends the MLP and the residual stream: the GELU epilogue of every GEMM kernel
(bf16 and MXFP8, plain and GELU -> MX), the gated-residual epilogue of every bf16 GEMM kernel, and both SiLU forms (gemv.hip,
gn_apply_kernel) - against the fp64 references and with the bounds of tests/value_sweep_refs.py, which have no absolute allowance.
tests/test_value_sweep_refs_cpu.py shows without a GPU that an fp32 emulation of each form passes them and subtly wrong forms fail.

A 0/1 weight matrix carries A[m, k(n)] into C[m, n] exactly (value_sweep_refs.carrier); EPI_NONE proves that per kernel first
(_delivered), and every later sweep takes its input values from what that step saw delivered.  Outputs live in NaN-sentinel guard
windows (dit_refs.guarded); every force knob is restored in a `finally`.  `-s` prints one `value-sweep` line per case.

Measured on MI355X (profiles/value_sweep_parity.txt, one line per case):
  * denormals: every site KEEPS the 254 bf16 denormals - the 128 x 128, 256 x 256 streamed, 144-row and 384-row kernels, the
    few-token kernel in both tile shapes, and the split-K slices on the 128 x 128, the 256-row (weight ring and 2 + 2 stage) and the
    few-token kernels all deliver them bit for bit under EPI_NONE (flushed 0 of 254), as do gemv (ACT_NONE) and GroupNorm (silu = 0).
    -0 arrives as +0 everywhere (the fp32 sum starts from +0).  No input is excluded from the later sweeps.
    A known hole: a product cannot carry -0, so no GEMM epilogue is seen with a -0 input here (gemv's SiLU and GroupNorm's take
    their value without a product in front, but the sum behind / the + beta turns -0 into +0 there too).
  * GELU, all twelve bf16 sites and the MXFP8 kernels (256 x 256, ring 256 x 64, ring 128 x 128; plain and GELU -> MX): worst 0.531
    ulp for x >= -4.5 - the figure the CPU emulation of gelu_erf_fast gives, to the digit; bit-equal share on the live range (2^-10 <= |x| < 8,
    x >= -4.5: 3217 values) 0.9938 .. 0.9947 against torch fp32's 0.9953 .. 0.9959 on the same elements - the emulation's 3200 and
    torch's 3203 of 3217, weighted by how often a case carries each value (MXFP8's 12 binades: 0.9952 against 0.9948); every site
    the same bits per value.
    (torch's own fp32 formula, held to the 1-ulp bound, misses it at x = -4.40625 and -4.46875: 1.6 ulp.)
  * gated residual, apart and aliased: bit-equal to torch's bf16 chain res + gate * lin at every site (the 384-row kernel with one clip and, at 768 rows, with two); 1.36 .. 1.40 % excluded.
  * SiLU: gemv 0.500 ulp, share 1.0 (torch 1.0), with and without a power-of-two mul; GroupNorm row and generic kernel 0.500 ulp,
    share 0.99998 (torch 1.0).

The MXFP8 sweep covers 2^-8 <= |v| < 16 as the range is stated: 12 binades, 3072 values (768 rows x 4 pairs of K blocks).  The
existing MXFP8 GEMM tests (tests/test_mx_gemm_edges_gpu.py) carry no availability check - the kernels are built for every gfx950
library - so none guards these either; the `mx_hooks` fixture mirrors their `hooks`.
"""
import pytest
import torch

import dit_refs as R
import mx_emul as MX
import value_sweep_refs as V
from test_gemm_plan_cpu import describe

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
SITES = pytest.mark.parametrize("s", V.GEMM_SITES, ids=lambda s: s.name)


def _ok(f, site):
    print(V.line(site, f))
    assert not f.failures, (site, f.failures)


# ------------------------------------------------------------------------------------------------ one launch of a site
def _launch(pkg, gpu, s, launch, epi, gate=None, res=None, alias=False):
    """One product of site s (its launch `launch` of the sweep) into a fresh guarded window.  Returns (C window, intended bits on
    the GPU)."""
    N_ = pkg.native
    lib = N_.load_library()
    a, w, intended = V.carrier(s, launch)
    ad, wd = a.to(gpu), w.to(gpu)
    ldc = s.N + 64
    cbuf, cv = R.guarded(s.M, s.N, ldc, 2, gpu)
    guards = [(cbuf, cv)]
    kw = dict(rows_per_batch=s.rpb, splitk=s.splitk)
    ldr, rv = s.N, None
    if epi == R.EPI_GATE_RES:
        if alias:
            cv.copy_(res)
            rv, ldr = cv, ldc
        else:
            ldr = s.N + 128
            rbuf, rv = R.guarded(s.M, s.N, ldr, 2, gpu)
            rv.copy_(res)
            guards.append((rbuf, rv))
        kw.update(gate=gate.to(gpu), residual=rv)
    if s.force >= 0:
        lib.drn_gemm_force_tile(s.force)
    if s.tall >= 0:
        lib.drn_gemm_tall_force_shape(s.tall)
    try:
        if s.splitk is None:
            assert lib.drn_gemm_splitk_choice(N_._clip_rows(s.M, s.rpb), s.N, s.K) == s.splits, "the site must run as listed"
        plan = describe(lib, s.M, s.N, s.K, ld=(s.K, s.K, ldc, ldr), epi=epi, rpb=s.rpb, splits=s.splits)
        assert plan is not None and len(plan) == 1 and plan[0][0] == s.kernel and plan[0][2] == s.M, (s.name, plan)
        N_.gemm(ad, wd, out=cv, epilogue=epi, **kw)
        torch.cuda.synchronize()
    finally:
        lib.drn_gemm_force_tile(-1)
        lib.drn_gemm_tall_force_shape(-1)
    for buf, v in guards:
        R.assert_guard_intact(buf, v)
    if rv is not None and not alias:
        assert torch.equal(rv, res.to(gpu)), "the residual is an input: not written"
    return cv, intended.to(gpu)


def _table_put(tab, keys, vals, what):
    """tab[key] = val for a launch's elements; a key must map to ONE value, within the launch and against earlier launches."""
    prev = tab[keys]
    assert bool(((prev < 0) | (prev == vals)).all()), f"{what}: one value, two results (against an earlier launch)"
    tab[keys.flatten()] = vals.flatten()
    bad = tab[keys] != vals
    assert not bool(bad.any()), f"{what}: one value, two results in one launch; first (m, n) {bad.nonzero()[:4].tolist()}"


_DELIVERED = {}


def _delivered(pkg, gpu, s):
    """EPI_NONE at site s: (table [65536] int64: the bits C held for each value of the sweep, flushed [65536] bool).  Asserts that
    every normal value arrives bit for bit, a zero as a zero, a denormal as itself or as a zero.  Run once per site and session."""
    if s.name in _DELIVERED:
        return _DELIVERED[s.name]
    tab = torch.full((65536,), -1, dtype=torch.int64, device=gpu)
    for launch in range(V.site_launches(s)):
        out, ib = _launch(pkg, gpu, s, launch, R.EPI_NONE)
        left = R.is_sentinel(out)
        assert not bool(left.any()), f"{int(left.sum())} cells never written; first (m, n) {left.nonzero()[:4].tolist()}"
        _table_put(tab, ib, V.bits_of_bf16(out).view(s.M, s.N), f"{s.name} EPI_NONE")
    sw = V.sweep_values().to(gpu)
    got = tab[sw]
    assert bool((got >= 0).all()), "a value of the sweep was never carried"
    zero_out = V.is_zero_bits(got)
    normal = ~V.is_zero_bits(sw) & ~V.is_denormal_bits(sw)
    bad = normal & (got != sw)
    assert not bool(bad.any()), (f"{s.name}: {int(bad.sum())} normal values not carried bit for bit; first "
                                 f"{[(hex(a), hex(b)) for a, b in zip(sw[bad][:4].tolist(), got[bad][:4].tolist())]}")
    assert bool(zero_out[V.is_zero_bits(sw)].all()), "a zero must arrive as a zero"
    den = V.is_denormal_bits(sw)
    assert bool(((got == sw) | zero_out)[den].all()), "a denormal arrives as itself or as a zero"
    flushed = torch.zeros(65536, dtype=torch.bool, device=gpu)
    flushed[sw[den & (got != sw)]] = True
    print(f"value-sweep none {s.name}: {int(normal.sum())} normal values bit-exact; denormals kept {int((den & (got == sw)).sum())} "
          f"flushed {int(flushed.sum())}; -0 arrives as {hex(int(tab[0x8000]))}")
    _DELIVERED[s.name] = (tab, flushed)
    return _DELIVERED[s.name]


# ------------------------------------------------------------------------------------------------ EPI_NONE
@SITES
def test_carrier_is_exact_on_every_kernel(pkg, gpu, s):
    """Normal values and zeros bit for bit; a denormal as itself or as a zero (recorded in the module docstring, not asserted:
    whether the matrix pipe keeps bf16 denormals is the hardware's business)."""
    _delivered(pkg, gpu, s)                               # (the assertions are _delivered's own)


# ------------------------------------------------------------------------------------------------ EPI_GELU
_GELU_TABLE = {}


def _gelu_site(pkg, gpu, s):
    """The GELU sweep of site s: every bound of value_sweep_refs.gelu_check; returns the table value bits -> output bits."""
    if s.name in _GELU_TABLE:
        return _GELU_TABLE[s.name]
    tab, flushed = _delivered(pkg, gpu, s)
    gt = torch.full((65536,), -1, dtype=torch.int64, device=gpu)
    for launch in range(V.site_launches(s)):
        out, ib = _launch(pkg, gpu, s, launch, R.EPI_GELU)
        xb = tab[ib]
        _ok(V.gelu_check(xb, out, excluded=flushed[ib]), f"gelu {s.name}" + (f" launch {launch}" if launch else ""))
        _table_put(gt, xb, V.bits_of_bf16(out).view(s.M, s.N), f"{s.name} EPI_GELU")
    _GELU_TABLE[s.name] = gt
    return gt


def _same_gelu_bits(gt, ref, what):
    both = (gt >= 0) & (ref >= 0)
    bad = both & (gt != ref)
    assert int(both.sum()) >= 3072
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} values leave this GELU site with other bits than the 128 x 128 kernel; "
                                 f"first value bits {[hex(v) for v in bad.nonzero().flatten()[:6].tolist()]}")


@SITES
def test_gelu_every_value(pkg, gpu, s):
    gt = _gelu_site(pkg, gpu, s)
    # one device function ends every kernel: the same value must leave every site with the same bits
    _same_gelu_bits(gt, _gelu_site(pkg, gpu, V.SITE_BY_NAME["k128"]), s.name)


# ------------------------------------------------------------------------------------------------ EPI_GATE_RES
@pytest.mark.parametrize("alias", [False, True], ids=["apart", "aliased"])
@SITES
def test_gated_residual_every_value(pkg, gpu, s, alias):
    tab, flushed = _delivered(pkg, gpu, s)
    gate = V.gate_rows_of(s)
    rows = V.expand_gate(gate.to(gpu), s.M, s.rpb)
    for launch in range(V.site_launches(s)):
        res = V.residual_of(s, launch)
        out, ib = _launch(pkg, gpu, s, launch, R.EPI_GATE_RES, gate, res, alias)
        lin = V.bf16_of_bits(tab[ib])
        f = V.gate_res_check(out, lin, rows, res.to(gpu), excluded=flushed[ib])
        _ok(f, f"gate_res {s.name} {'aliased' if alias else 'apart'}" + (f" launch {launch}" if launch else ""))


# ------------------------------------------------------------------------------------------------ MXFP8
MX_SITES = (("mx-k256", -1), ("mx-ring0", 0), ("mx-ring1", 1))


@pytest.fixture()
def mx_hooks(pkg, gpu):
    lib = pkg.native.load_library()
    was = lib.drn_gemm_mxfp8_force_small_m(1)
    shape = lib.drn_gemm_mxfp8_tall_force_shape(-1)
    try:
        yield lib
    finally:
        lib.drn_gemm_mxfp8_force_small_m(was)
        lib.drn_gemm_mxfp8_tall_force_shape(shape)


def _mx_launch(pkg, gpu, lib, shape, epi, out_mx=False):
    """The MX carrier on drn_gemm_mxfp8 (shape -1) or the few-token ring kernel of that tile shape, unsplit."""
    N_ = pkg.native
    c = V.mx_carrier()
    a, w = N_.MxTensor(c.aq.to(gpu), c.sa.to(gpu)), N_.MxTensor(c.wq.to(gpu), c.sw.to(gpu))
    if shape >= 0:
        lib.drn_gemm_mxfp8_tall_force_shape(shape)
    if out_mx:
        lib.drn_gemm_mxfp8_force_small_m(1 if shape >= 0 else 0)
        assert N_.mx_gemm_plan(V.MX_M, V.MX_N, V.MX_K, V.MX_RPB) == (1 if shape >= 0 else 0), "the form must take the kernel it is listed under"
        qb, qv = R.guarded(V.MX_M, V.MX_N, V.MX_N, 2, gpu, dtype=torch.uint8)
        sb, sv = R.guarded(V.MX_M, V.MX_N // 32, V.MX_N // 32, 4, gpu, dtype=torch.uint8)
        N_.gemm_mxfp8(a, w, epilogue=epi, rows_per_batch=V.MX_RPB, out_mx=N_.MxTensor(qv.view(F8), sv))
        torch.cuda.synchronize()
        R.assert_guard_intact(qb, qv)
        R.assert_guard_intact(sb, sv)
        return qv, sv
    cbuf, cv = R.guarded(V.MX_M, V.MX_N, V.MX_N + 64, 2, gpu)
    N_.gemm_mxfp8(a, w, out=cv, epilogue=epi, rows_per_batch=V.MX_RPB, splitk=0 if shape < 0 else 1)
    torch.cuda.synchronize()
    R.assert_guard_intact(cbuf, cv)
    return cv


@pytest.mark.parametrize("name,shape", MX_SITES, ids=[n for n, _ in MX_SITES])
def test_mx_gelu_every_value_of_twelve_binades(pkg, gpu, mx_hooks, name, shape):
    """hi + lo in two K blocks carry 3072 values into the MXFP8 kernels' epilogues: exact with EPI_NONE; the plain GELU within the
    bounds and with the bits of the bf16 kernels; the GELU -> MX form = mx_emul's quantisation of those bits (include/drn.h)."""
    ib = V.mx_carrier().intended.to(gpu)
    lin = _mx_launch(pkg, gpu, mx_hooks, shape, R.EPI_NONE)
    bad = V.bits_of_bf16(lin).view(ib.shape) != ib
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} values not carried bit for bit; first (m, n) {bad.nonzero()[:4].tolist()}"
    out = _mx_launch(pkg, gpu, mx_hooks, shape, R.EPI_GELU)
    _ok(V.gelu_check(ib, out), f"gelu {name}")
    gt = torch.full((65536,), -1, dtype=torch.int64, device=gpu)
    _table_put(gt, ib, V.bits_of_bf16(out).view(ib.shape), f"{name} EPI_GELU")
    _same_gelu_bits(gt, _gelu_site(pkg, gpu, V.SITE_BY_NAME["k128"]), name)
    q, sc = _mx_launch(pkg, gpu, mx_hooks, shape, R.EPI_GELU, out_mx=True)
    want_q, want_s = MX.quantize(out.cpu().contiguous())
    assert not bool(R.is_sentinel(sc.cpu()).any()), "a scale byte was never written"
    assert torch.equal(sc.cpu(), want_s), f"{name}: {int((sc.cpu() != want_s).sum())} scale bytes differ from quantize(bf16 GELU)"
    diff = q.cpu() != want_q.view(torch.uint8)
    assert not bool(diff.any()), f"{name}: {int(diff.sum())} element bytes differ from quantize(bf16 GELU); first {diff.nonzero()[:4].tolist()}"
    print(f"value-sweep gelu-mx {name}: {q.numel()} bytes and {sc.numel()} scales bit-equal to quantize(bf16 GELU)")


# ------------------------------------------------------------------------------------------------ SiLU: gemv
GEMV_G, GEMV_B, GEMV_K = 4, 16, 1024           # 4 groups x 16 vectors x 1024 = 65 536 slots; K = 1024: two trips of the lane loop


def _gemv_inputs():
    sw = V.sweep_values()
    xb = sw[torch.arange(GEMV_G * GEMV_B * GEMV_K) % V.N_FINITE].view(GEMV_G, GEMV_B, GEMV_K)
    n = torch.arange(GEMV_K)
    kn = torch.stack([(5 * n + 37 * g) % GEMV_K for g in range(GEMV_G)])           # a permutation per group
    w = torch.zeros((GEMV_G, GEMV_K, GEMV_K), dtype=BF)
    for g in range(GEMV_G):
        w[g, n, kn[g]] = 1.0
    intended = torch.stack([xb[g][:, kn[g]] for g in range(GEMV_G)])
    return V.bf16_of_bits(xb), w, intended


@pytest.mark.parametrize("with_mul", [False, True], ids=["plain", "mul-pow2"])
def test_gemv_silu_every_value(pkg, gpu, with_mul):
    """ACT_SILU on 0/1 weights: out[g, b, n] = bf16(silu(x[g, b, k_g(n)])), no `add`; `mul` absent, or a power of two (exact)."""
    x, w, intended = _gemv_inputs()
    ib = intended.to(gpu)
    got = V.bits_of_bf16(pkg.native.gemv(x.to(gpu), w.to(gpu), act=0)).view(ib.shape)
    den, zero = V.is_denormal_bits(ib), V.is_zero_bits(ib)
    assert torch.equal(got[~den & ~zero], ib[~den & ~zero]), "ACT_NONE carries every normal value bit for bit"
    assert bool(((got == ib) | V.is_zero_bits(got))[den | zero].all()), "zeros and denormals arrive as themselves or as a zero"
    print(f"value-sweep none gemv: denormals kept {int((den & (got == ib)).sum())} of {int(den.sum())} elements")
    mul = scale = None
    if with_mul:
        n = torch.arange(GEMV_K).view(1, 1, -1) + torch.arange(GEMV_B).view(1, -1, 1)
        mul = torch.ldexp(torch.ones(1, GEMV_B, GEMV_K), (n % 6 - 2).float()).to(BF).to(gpu)
        scale = mul.expand(GEMV_G, -1, -1)
    buf, win = R.guarded(GEMV_G * GEMV_B, GEMV_K, GEMV_K, 2, gpu)
    pkg.native.gemv(x.to(gpu), w.to(gpu), out=win.view(GEMV_G, GEMV_B, GEMV_K), mul=mul, act=1)
    torch.cuda.synchronize()
    R.assert_guard_intact(buf, win)
    # (SiLU is applied to x as it is loaded: a denormal x is not flushed by a product in front of it)
    _ok(V.silu_check(ib, win.view(GEMV_G, GEMV_B, GEMV_K), scale=scale), "silu gemv" + (" mul 2^k" if with_mul else ""))


# ------------------------------------------------------------------------------------------------ SiLU: GroupNorm
@pytest.mark.parametrize("C", [512, 192], ids=["rows-C512", "generic-C192"])
def test_groupnorm_silu_every_value(pkg, gpu, C):
    """An all-zero frame with gamma = 0: o = rbf(0 * 0 + beta) = beta reaches the SiLU exactly.  Four frames of 2 x 2 pixels per
    launch, C values per launch (beta is per channel): 128 launches of the row kernel at C = 512, 340 of the generic one at 192.
    With silu = 0 the output must be beta (the carrier); with silu = 1 the bounds of value_sweep_refs.silu_check."""
    Vn = pkg.native_vae
    T_, H, W = 4, 2, 2
    sw = V.sweep_values()
    L = -(-V.N_FINITE // C)
    bb = sw[torch.arange(L * C) % V.N_FINITE].view(L, C).to(gpu)
    beta = V.bf16_of_bits(bb)
    gamma = torch.zeros(C, dtype=BF, device=gpu)
    x = Vn.CL(T_, H, W, C, 1, gpu, tensor=torch.zeros((T_, H + 2, W + 2, C), dtype=BF, device=gpu))
    ib = bb.view(L, 1, 1, 1, C).expand(L, T_, H, W, C)
    delivered = None
    for silu in (False, True):
        y = torch.zeros((L, T_, H + 2, W + 2, C), dtype=BF, device=gpu)
        for l in range(L):
            Vn.groupnorm_silu(x, gamma, beta[l], silu, out=Vn.CL(T_, H, W, C, 1, gpu, tensor=y[l]))
        torch.cuda.synchronize()
        inner = y[:, :, 1:1 + H, 1:1 + W, :]
        halo = y.clone()
        halo[:, :, 1:1 + H, 1:1 + W, :] = 0
        assert not bool(halo.any()), "halo written"
        if not silu:
            got = V.bits_of_bf16(inner).view(ib.shape)
            keep = ~V.is_zero_bits(ib) & ~V.is_denormal_bits(ib)
            bad = keep & (got != ib)
            assert not bool(bad.any()), f"{int(bad.sum())} normal values do not reach the output as beta"
            assert bool(((got == ib) | V.is_zero_bits(got))[~keep].all()), "zeros and denormals arrive as themselves or as a zero"
            den = V.is_denormal_bits(ib)
            print(f"value-sweep none groupnorm C{C}: denormals kept {int((den & (got == ib)).sum())} of {int(den.sum())} elements")
            delivered = got
        else:
            _ok(V.silu_check(delivered, inner, excluded=V.is_denormal_bits(ib) & (delivered != ib)), f"silu groupnorm C{C}")


# ------------------------------------------------------------------------------------------------ last
def test_value_sweep_leaves_no_knob_behind(pkg, gpu):
    """The last test of the module: what test_dit_kernel_edges_gpu.test_force_knobs_are_back_at_their_defaults reads."""
    lib = pkg.native.load_library()
    assert lib.drn_gemm_tall_force_shape(-1) == -1
    assert lib.drn_gemm_tile_choice(18432, 16384) == 1 and lib.drn_gemm_tile_choice(2304, 4096) == 2
    assert lib.drn_gemm_splitk_choice(256, 4096, 16384) == 16
    assert lib.drn_gemm_mxfp8_tall_force_shape(-1) == -1
