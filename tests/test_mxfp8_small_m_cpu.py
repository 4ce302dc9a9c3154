"""MXFP8 at few tokens, host side (no GPU): the choice function of the few-token MXFP8 GEMM, its tuning hook, the sizers of
drn_dit_forward with precision 1 and the refusals that function makes before it launches anything."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

CFG1 = [(12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384)]       # q|k|v, out-proj, MLP-up, MLP-down at D = 4096
SHAPES = CFG1 + [(256, 256), (512, 2048), (1024, 256), (3072, 1024), (768, 512)]


@pytest.fixture()
def lib(pkg):
    lib = pkg.native.load_library()
    was = lib.drn_gemm_mxfp8_force_small_m(1)
    yield lib
    lib.drn_gemm_mxfp8_force_small_m(was)


def test_new_symbols_declared_bound_and_exported(pkg, lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drn.h")).read(), flags=re.S)
    for name in ("drn_gemm_mxfp8_splitk_choice", "drn_gemm_mxfp8_force_small_m", "drn_gemm_mxfp8_splitk",
                 "drn_gemm_mxfp8_splitk_partials", "drn_dit_forward_mx_act_bytes", "drn_dit_forward_mx_gemm_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in pkg.native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.drn_abi_version() == 1


def test_choice_rule(pkg, lib):
    ch = lib.drn_gemm_mxfp8_splitk_choice
    for N, K in CFG1:
        assert ch(256, N, K) >= 1, (N, K)
        assert ch(18432, N, K) == 0, (N, K)
    assert ch(256, 4096 + 128, 4096) == 0          # N % 256
    assert ch(256, 4096, 4096 + 64) == 0           # K % 128
    assert ch(256 + 128, 4096, 4096) == 0          # M % 256
    assert ch(100, 4096, 4096) == 0 and ch(1280, 4096, 4096) == 0 and ch(0, 4096, 4096) == 0
    for M in (256, 512, 768, 1024):
        for N, K in SHAPES:
            s = ch(M, N, K)
            assert 0 <= s <= 64 and (s == 0 or (K // 128) % s == 0), (M, N, K, s)
            if s == 0:                    # only where the 256 x 256 tiles of drn_gemm_mxfp8 fill most of the chip themselves
                assert (M // 256) * (N // 256) >= 192, (M, N, K)
                continue
            # decomposition first: a sliced product covers at most one round of the 256 CUs and keeps the ring fed
            tiles = M * N // 16384
            assert s == 1 or (tiles * s <= 256 and K // 128 // s >= 8), (M, N, K, s)
            # and a product is not left on fewer than half of the CUs while its K is long enough to cut again
            assert tiles * s > 128 or K // 128 // (2 * s) < 8 or (K // 128) % (2 * s), (M, N, K, s)
    # the out-projection and MLP-down of cfg 1 (64 column tiles) are sliced; q|k|v and MLP-up fill the chip unsplit
    assert ch(256, 12288, 4096) == 1 and ch(256, 16384, 4096) == 1
    assert ch(256, 4096, 4096) > 1 and ch(256, 4096, 16384) > 1


def test_plan_is_that_of_one_clip(pkg, lib):
    N = pkg.native
    for n, k in SHAPES:
        assert N.mx_gemm_plan(2 * 256, n, k, rows_per_batch=256) == N.mx_gemm_plan(256, n, k, None)
        assert N.mx_gemm_plan(3 * 512, n, k, rows_per_batch=512) == N.mx_gemm_plan(512, n, k, None)
        assert N.mx_gemm_plan(256, n, k, None) == lib.drn_gemm_mxfp8_splitk_choice(256, n, k)
    assert N.mx_gemm_plan(72 * 256, 4096, 4096, rows_per_batch=18432) == 0


def test_hook_switches_the_choice_off(pkg, lib):
    assert lib.drn_gemm_mxfp8_force_small_m(-1) == 1                  # query only
    assert lib.drn_gemm_mxfp8_force_small_m(0) == 1                   # returns the previous setting
    try:
        assert lib.drn_gemm_mxfp8_force_small_m(-1) == 0
        for M in (256, 512, 1024, 18432):
            for n, k in SHAPES:
                assert lib.drn_gemm_mxfp8_splitk_choice(M, n, k) == 0
                assert pkg.native.mx_gemm_plan(M, n, k) == 0
        assert lib.drn_dit_forward_mx_gemm_workspace_bytes(1, 256, 4096, 16384) == 0
    finally:
        assert lib.drn_gemm_mxfp8_force_small_m(1) == 0
    assert lib.drn_gemm_mxfp8_splitk_choice(256, 4096, 4096) >= 1


def test_forward_sizers(pkg, lib):
    for B, S, D, hidden in [(1, 256, 4096, 16384), (2, 256, 4096, 16384), (1, 1024, 4096, 16384), (1, 18432, 4096, 16384),
                            (3, 512, 1024, 4096), (1, 128, 512, 2048)]:
        k = max(D, hidden)
        assert lib.drn_dit_forward_mx_act_bytes(B, S, D, hidden) >= B * S * k + B * S * k // 32
        need = lib.drn_dit_forward_mx_gemm_workspace_bytes(B, S, D, hidden)
        for n, kk in [(3 * D, D), (D, D), (hidden, D), (D, hidden)]:
            s = lib.drn_gemm_mxfp8_splitk_choice(S, n, kk)
            assert need >= lib.drn_gemm_splitk_workspace_bytes(B * S, n, s), (B, S, n, kk, s)
    # cfg 1: the sliced out-projection / MLP-down write [s][256][4096] fp32
    s = lib.drn_gemm_mxfp8_splitk_choice(256, 4096, 16384)
    assert lib.drn_dit_forward_mx_gemm_workspace_bytes(1, 256, 4096, 16384) >= s * 256 * 4096 * 4


def _mx_args(pkg, lib, B=1, S=256, D=4096, hidden=16384):
    """drn_dit_forward_args of an MXFP8 forward that passes every check (fake, never dereferenced device addresses)."""
    N = pkg.native
    fake = 1 << 20
    subs = (N.DitSub * 2)()
    subs[0].kind, subs[0].site, subs[0].ca_index = N.SUB_FA, 0, -1
    subs[1].kind, subs[1].site, subs[1].ca_index = N.SUB_MLP, 1, -1
    for e in subs:
        e.w_a = e.w_b = e.s_a = e.s_b = e.qn = e.kn = fake
    a = N.DitForwardArgs()
    a.struct_bytes = ctypes.sizeof(N.DitForwardArgs)
    a.S, a.B, a.D, a.hidden, a.heads = S, B, D, hidden, D // 128
    a.n_sub, a.subs = 2, subs
    for f in ("shift", "scale", "gate", "cos", "sin", "P", "w_patch", "final_shift", "final_scale", "w_final",
              "X", "H", "QKV", "O", "U", "Y", "gemm_ws", "attn_ws", "AQ", "AS"):
        setattr(a, f, fake)
    a.kpad, a.n_final = 192, 128
    a.gemm_ws_bytes = max(lib.drn_dit_forward_gemm_workspace_bytes(B, S, D, hidden, 128, 192),
                          lib.drn_dit_forward_mx_gemm_workspace_bytes(B, S, D, hidden))
    a.attn_ws_bytes = 1 << 40
    a.act_bytes = lib.drn_dit_forward_mx_act_bytes(B, S, D, hidden)
    a.eps, a.precision = 1e-6, 1
    return a, subs


def test_forward_refuses_before_any_launch(pkg, lib):
    """Every refusal below is decided on the host from the argument block alone: DRN_EINVAL (-1), nothing enqueued."""
    N = pkg.native
    fwd = lib.drn_dit_forward

    a, subs = _mx_args(pkg, lib)
    a.AQ = None
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = _mx_args(pkg, lib)
    a.AS = None
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = _mx_args(pkg, lib)
    a.act_bytes -= 1
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = _mx_args(pkg, lib)
    a.gemm_ws_bytes = lib.drn_dit_forward_mx_gemm_workspace_bytes(1, 256, 4096, 16384) - 1
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = _mx_args(pkg, lib)
    a.gemm_ws = None
    assert fwd(ctypes.byref(a), None) == -1
    for field in ("s_a", "s_b"):
        for i in (0, 1):
            a, subs = _mx_args(pkg, lib)
            setattr(subs[i], field, None)
            assert fwd(ctypes.byref(a), None) == -1, (field, i)
    a, subs = _mx_args(pkg, lib)
    a.precision = 2
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = _mx_args(pkg, lib, D=4096 + 128)              # D % 256
    assert fwd(ctypes.byref(a), None) == -1


def test_forward_refuses_per_sub_block_faults_before_any_launch(pkg, lib):
    """What a sub-block or the attention plan needs is checked with everything else, before the patch-embed GEMM is enqueued (without
    a GPU a launch would return a positive hipError_t, so -1 can only come from a check that ran first).  Both precisions."""
    N = pkg.native
    fwd = lib.drn_dit_forward

    def args(precision, **kw):
        a, subs = _mx_args(pkg, lib, **kw)
        a.precision = precision
        a.addvec, a.addvec_stride = 1 << 20, a.D
        return a, subs

    def not_refused(a):
        """Valid args get past validate(): without a GPU the first launch then fails with a positive hipError_t.  Only asked
        where no GPU is visible - with one, the call would enqueue kernels on the fake addresses."""
        import torch
        return torch.cuda.is_available() or fwd(ctypes.byref(a), None) > 0

    for precision in (0, 1):
        # controls: the unchanged args pass every check, so each -1 below comes from the one thing changed
        a, subs = args(precision)
        assert not_refused(a)
        a, subs = args(precision)
        subs[1].kind, subs[1].ca_index = N.SUB_CA, 0
        assert not_refused(a)
        a, subs = args(precision)
        subs[1].kind = 7
        assert fwd(ctypes.byref(a), None) == -1
        a, subs = args(precision)
        subs[0].qn = None
        assert fwd(ctypes.byref(a), None) == -1
        a, subs = args(precision)
        subs[1].kind, subs[1].ca_index = N.SUB_CA, 0
        a.addvec = None
        assert fwd(ctypes.byref(a), None) == -1
        # 4 heads, 16 640 tokens: the plan's second launch splits its keys and needs the split-KV workspace
        a, subs = args(precision, S=16640, D=512, hidden=2048)
        need = lib.drn_dit_forward_attn_workspace_bytes(1, 4, 16640)
        assert need > 0 and N.attention_plan(1, 4, 16640, 16640) == [(0, 16384, 1), (16384, 16640, 8)]
        a.attn_ws_bytes = need
        assert not_refused(a)                                                    # control: exactly enough
        a.attn_ws_bytes = need - 1
        assert fwd(ctypes.byref(a), None) == -1
        a.attn_ws_bytes, a.attn_ws = need, None
        assert fwd(ctypes.byref(a), None) == -1


def test_split_entry_points_refuse_on_the_host(pkg, lib):
    """The contract of drn_gemm_mxfp8_splitk / _partials is checked before the launch: these calls need no GPU."""
    p = 1 << 20
    sk, pt = lib.drn_gemm_mxfp8_splitk, lib.drn_gemm_mxfp8_splitk_partials

    def call(M=256, N=512, K=1024, splits=2, ws=p, rpb=0):
        return sk(p, p, p, p, p, M, N, K, N, 0, None, None, 0, rpb, splits, ws, None)

    assert call(M=256 + 64) == -1                 # M % 256
    assert call(N=512 + 128) == -1                # N % 256
    assert call(K=1024 + 64) == -1                # K % 128
    assert call(splits=3) == -1                   # 3 does not divide K / 128 = 8
    assert call(K=128 * 128, splits=128) == -1    # > 64
    assert call(splits=0) == -1
    assert call(ws=None) == -1                    # slices need a workspace
    assert call(M=2048) == -1 and call(M=4096, rpb=2048) == -1      # more than 1024 rows per clip
    assert pt(p, p, p, p, 256, 512, 1024, 0, 1, p, None) == -1      # the slices alone: splits >= 2
    assert pt(p, p, p, p, 256, 512, 1024, 0, 2, None, None) == -1
    assert pt(p, p, p, p, 256 + 64, 512, 1024, 0, 2, p, None) == -1
