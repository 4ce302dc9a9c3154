"""The HBM-bound passes of a DiT block on their many-rows paths, one row past 4096 (D = 4096, 32 heads): ln_modulate without and
with the pending add, and q/k norm + RoPE with more work items than its grid has waves, so the grid-stride loop runs with a ragged
tail.  Each equals, bit for bit, the same entry point called row by row (for
ln_modulate that is four waves per row, the few-rows kernel: one summation tree, csrc/elementwise.hip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, D, HEADS = 4097, 4096, 32
RPB = 2049                      # two clips (2049 + 2048 rows): shift / scale / add change inside the launch


def _rnd(gpu, seed, *shape, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(gpu)


@pytest.fixture(scope="module")
def ln_case(pkg, gpu):
    """x, the per-clip vectors and the row-by-row results (h without add; x and h with it), computed once."""
    N, lib = pkg.native, pkg.native.load_library()
    x = _rnd(gpu, 1, M, D, scale=3.0)
    x[7] = 0                                                # a constant row: variance 0
    shift, scale, add = _rnd(gpu, 2, 2, D), _rnd(gpu, 3, 2, D), _rnd(gpu, 4, 2, D)
    ref = {}
    lib.drn_ln_force_kernel(1)
    try:
        for with_add in (False, True):
            xr, h = x.clone(), torch.empty_like(x)
            for r in range(M):
                b = r // RPB
                N.ln_modulate(xr[r:r + 1], shift[b:b + 1], scale[b:b + 1], out=h[r:r + 1], add_vec=add[b:b + 1] if with_add else None)
            ref[with_add] = (xr, h)
    finally:
        lib.drn_ln_force_kernel(-1)
    torch.cuda.synchronize()
    assert torch.equal(ref[False][0], x) and not torch.equal(ref[True][0], x)
    return x, shift, scale, add, ref


@pytest.mark.parametrize("force", [-1, 0], ids=["launchers_choice", "one_wave_per_row"])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "pending_add"])
def test_ln_modulate_many_rows(pkg, ln_case, with_add, force):
    N, lib = pkg.native, pkg.native.load_library()
    x, shift, scale, add, ref = ln_case
    xm, h = x.clone(), torch.full_like(x, float("nan"))
    lib.drn_ln_force_kernel(force)
    try:
        N.ln_modulate(xm, shift, scale, out=h, add_vec=add if with_add else None, rows_per_batch=RPB)
    finally:
        lib.drn_ln_force_kernel(-1)
    torch.cuda.synchronize()
    assert torch.equal(xm, ref[with_add][0])
    assert torch.equal(h, ref[with_add][1])


def test_qk_norm_rope_many_rows(pkg, gpu):
    N = pkg.native
    qkv = _rnd(gpu, 5, M, 3 * D, scale=2.0)
    wq, wk = _rnd(gpu, 6, 128), _rnd(gpu, 7, 128)
    cos, sin = _rnd(gpu, 8, RPB, 128), _rnd(gpu, 9, RPB, 128)
    assert M * (HEADS // 8) * 2 > 8192 * 4                  # more items than the capped grid has waves
    many = qkv.clone()
    N.qk_norm_rope(many[:, :D], many[:, D:2 * D], wq, wk, cos, sin, HEADS, tokens_per_batch=RPB)
    rows = qkv.clone()
    for r in range(M):
        N.qk_norm_rope(rows[r:r + 1, :D], rows[r:r + 1, D:2 * D], wq, wk, cos, sin, HEADS, tokens_per_batch=RPB, pos_offset=r % RPB)
    torch.cuda.synchronize()
    assert torch.equal(many[:, 2 * D:], qkv[:, 2 * D:])      # V untouched
    assert torch.equal(many, rows) and not torch.equal(many, qkv)
