"""MXFP8 under sequence parallelism, host side (no GPU): the refusals drn_gemm_mxfp8_blocked makes before it launches anything,
and the plane-address rule of its binding at the slab shapes of the head <-> token all-to-all."""
import os
import re

import pytest
import torch

from conftest import ROOT

EINVAL = -1
M, N, K = 300, 512, 256
# fake, suitably aligned device addresses: every call below must be refused on the host, before a pointer is ever used
A, SA, W, SW, C, G, R = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


@pytest.fixture()
def lib(pkg):
    return pkg.native.load_library()


def test_symbol_declared_bound_and_exported(pkg, lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drn.h")).read(), flags=re.S)
    assert re.search(r"\bdrn_gemm_mxfp8_blocked\s*\(", text)
    assert len(pkg.native.SIGNATURES["drn_gemm_mxfp8_blocked"]) == 19
    assert hasattr(lib, "drn_gemm_mxfp8_blocked")


def _call(lib, **kw):
    a = dict(A=A, SA=SA, W=W, SW=SW, C=C, M=M, N=N, K=K, ldc=N, epi=0, gate=None, res=None, ldr=0, rpb=M,
             abc=0, abs_=0, cbc=0, cbs=0)
    a.update(kw)
    return lib.drn_gemm_mxfp8_blocked(a["A"], a["SA"], a["W"], a["SW"], a["C"], a["M"], a["N"], a["K"], a["ldc"], a["epi"], a["gate"],
                                      a["res"], a["ldr"], a["rpb"], a["abc"], a["abs_"], a["cbc"], a["cbs"], None)


A_OK = dict(abc=128, abs_=M * 128)
C_OK = dict(cbc=256, cbs=M * 256, ldc=256)

REFUSED = {
    # the contract of drn_gemm_mxfp8
    "null A": dict(A=None), "null SA": dict(SA=None), "null W": dict(W=None), "null SW": dict(SW=None), "null C": dict(C=None),
    "M = 0": dict(M=0), "N % 256": dict(N=384), "N < 256": dict(N=128), "K % 128": dict(K=192), "K < 128": dict(K=64),
    "ldc < N": dict(ldc=N - 4), "ldc % 4": dict(ldc=N + 2),
    "A misaligned": dict(A=A + 8), "W misaligned": dict(W=W + 8), "SA misaligned": dict(SA=SA + 2), "SW misaligned": dict(SW=SW + 1),
    "C misaligned": dict(C=C + 4), "epilogue": dict(epi=3), "the internal GELU -> MX epilogue": dict(epi=4),
    "gate missing": dict(epi=2, res=R, ldr=N), "residual missing": dict(epi=2, gate=G, ldr=N),
    "ldr < N": dict(epi=2, gate=G, res=R, ldr=N - 4), "residual misaligned": dict(epi=2, gate=G, res=R + 2, ldr=N),
    "gate misaligned": dict(epi=2, gate=G + 2, res=R, ldr=N),
    # A planes
    "a_block_cols 64": dict(abc=64, abs_=M * 64), "a_block_cols 96": dict(abc=96, abs_=M * 96),
    "K % a_block_cols": dict(K=384, abc=256, abs_=M * 256), "a_block_cols > K": dict(abc=512, abs_=M * 512),
    "a_block_cols < 0": dict(abc=-128, abs_=M * 128),
    "a_block_stride % 128": dict(abc=128, abs_=M * 128 + 64), "A planes overlap": dict(abc=128, abs_=(M - 1) * 128),
    "a_block_stride < 0": dict(abc=128, abs_=-M * 128),
    # C planes
    "c_block_cols 128": dict(cbc=128, cbs=M * 128, ldc=128), "c_block_cols 384 (no power of two)": dict(N=768, cbc=384, cbs=M * 384, ldc=384),
    "c_block_cols > N": dict(cbc=1024, cbs=M * 1024, ldc=1024), "c_block_cols < 0": dict(cbc=-256, cbs=M * 256, ldc=256),
    "ldc < c_block_cols": dict(cbc=256, cbs=M * 256, ldc=252), "c_block_stride % 4": dict(cbc=256, cbs=M * 256 + 2, ldc=256),
    "C planes overlap": dict(cbc=256, cbs=(M - 1) * 256 + 252, ldc=256), "c_block_stride < 0": dict(cbc=256, cbs=-M * 256, ldc=256),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_every_refusal_returns_before_a_launch(lib, what):
    """No GPU here and the pointers are fake: a call that got as far as a launch would return a HIP error (> 0) or fault,
    not DRN_EINVAL.  Each case breaks one rule of an otherwise valid call, alone and with the other operand in planes."""
    bad = REFUSED[what]
    assert _call(lib, **bad) == EINVAL, what
    for ok in (A_OK, C_OK):
        if not (set(ok) & set(bad)):
            assert _call(lib, **dict(ok, **bad)) == EINVAL, what


@pytest.mark.parametrize("world", [2, 4, 8])
def test_plane_args_of_the_slab_shapes(pkg, world):
    """The binding's plane rule at D = 4096: the send slabs of the K|V and Q projections (C planes) and the return slabs the
    out-projection reads (A planes: e4m3 bytes + scales) give the block_cols / block_stride drn.h documents."""
    Nn = pkg.native
    D, S = 4096, 18432
    rows, Wd = S // world, D // world
    dev = torch.device("meta")
    skv = torch.empty((world, rows, 2 * Wd), dtype=torch.bfloat16, device=dev)
    sq = torch.empty((world, rows, Wd), dtype=torch.bfloat16, device=dev)
    assert Nn.mx_plane_args(skv) == (2 * Wd, 2 * Wd, rows * 2 * Wd)
    assert Nn.mx_plane_args(sq) == (Wd, Wd, rows * Wd)
    oq = torch.empty((world, rows, Wd), dtype=torch.uint8, device=dev)
    osc = torch.empty((world, rows, Wd // 32), dtype=torch.uint8, device=dev)
    abc, lda, abs_ = Nn.mx_plane_args(oq)
    sbc, lds, sbs = Nn.mx_plane_args(osc)
    assert (abc, lda, abs_) == (Wd, Wd, rows * Wd) and (sbc, lds, sbs) == (Wd // 32, Wd // 32, rows * Wd // 32)
    # what the header asks of them: 128 | a_block_cols | K, the scale planes a_block_stride / 32 apart, C planes a power of two >= 256
    assert abc % 128 == 0 and D % abc == 0 and abs_ % 128 == 0 and abs_ >= rows * abc and sbs * 32 == abs_
    for cols in (Wd, 2 * Wd):
        assert cols >= 256 and cols & (cols - 1) == 0
    # a view with guard rows behind every plane keeps the row stride and widens the plane stride
    g = torch.empty((world, rows + 3, Wd), dtype=torch.uint8, device=dev)[:, :rows]
    assert Nn.mx_plane_args(g) == (Wd, Wd, (rows + 3) * Wd)
    # one plane: the stride of a size-1 dimension carries no meaning
    assert Nn.mx_plane_args(torch.empty((1, rows, D), dtype=torch.uint8, device=dev))[2] >= rows * D
