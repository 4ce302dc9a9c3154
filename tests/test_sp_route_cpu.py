"""The route of a sequence-parallel forward (dit_engine.sp_route), host side: no GPU and no engine, only the built library.
It is held to what tests/test_parallel_gpu.py and tests/test_mxfp8_parallel_gpu.py assert through `expect_path` / `sp_path` on
the GPU, at their geometries and under their force switches; nothing here is a new expectation."""
import contextlib

import pytest

TINY = (256, 2, 128)           # D, heads, S: tiny_net(pkg, 256, 2, 2) on a 2 x 16 x 16 latent
WIDE = (1024, 8, 2048)         # tiny_net(pkg, 1024, 1, 8) on 2 x 64 x 64
CLIP = (1024, 8, 18432)        # the same net on 8 x 72 x 128: the headline clip's token count


def _cases():
    """(geometry, world, exchange, mxfp8 linears, attention switch [+ drn_attention_mxfp8_force(1)], engine switches, sp_path)."""
    cases = []
    for mx in (False, True):
        for att in (False, True):
            a = "mxfp8" if att else "bf16"
            # tiny, 128 columns per rank: plain GEMM + regroup; mxfp8 linears: W // 32 = 4 scale bytes per row are no multiple of 16,
            # the regroup kernel cannot move them, so bf16 goes home.  128 tokens take the MXFP8 attention only when forced
            cases.append((TINY, 2, "a2a", mx, att, {}, ("regroup", "bf16", a)))
            cases.append((TINY, 2, "gather", mx, att, {}, ("gather", "none", a)))
            # wide: mxfp8 linears write / read the slabs through the blocked MXFP8 GEMM and return e4m3 at both worlds; bf16 linears
            # take the slabs from 512 columns per rank (world 2) and regroup at 256 (world 4)
            for world in (2, 4):
                slabs = mx or world == 2
                cases.append((WIDE, world, "a2a", mx, att, {}, ("slabs" if slabs else "regroup", "e4m3" if mx else "bf16", a)))
        cases.append((TINY, 4, "gather", mx, False, {}, ("gather", "none", "bf16")))
        cases.append((CLIP, 2, "a2a", mx, False, {}, ("slabs", "e4m3" if mx else "bf16", "bf16")))
        cases.append((CLIP, 2, "a2a", mx, False, {"split": False}, ("slabs", "e4m3" if mx else "bf16", "bf16")))
    cases.append((TINY, 2, "a2a", True, True, {"force_attn": False}, ("regroup", "bf16", "bf16")))     # below the 2048-token rule
    cases.append((WIDE, 2, "a2a", True, False, {"mx_return": False}, ("slabs", "bf16", "bf16")))      # DRN_SP_MX_RETURN=0
    return cases


CASES = _cases()


@contextlib.contextmanager
def _switches(pkg, geom, force_attn):
    """The force switches of the GPU tests' workers (_setup; `attn` mode), put back afterwards."""
    Nn, lib = pkg.native, pkg.native.load_library()
    small_m = attn = None
    try:
        if geom is not TINY:
            lib.drn_gemm_force_tile(1)
        small_m = lib.drn_gemm_mxfp8_force_small_m(0)
        if force_attn:
            attn = Nn.attention_mxfp8_force(1)
        yield
    finally:
        lib.drn_gemm_force_tile(-1)
        if small_m is not None:
            lib.drn_gemm_mxfp8_force_small_m(small_m)
        if attn is not None:
            Nn.attention_mxfp8_force(attn)


def _route(pkg, case):
    """sp_route as an engine of the case's precisions and switches asks it."""
    geom, world, exchange, mx, att, opt, _ = case
    with _switches(pkg, geom, att and opt.get("force_attn", True)):
        return pkg.dit_engine.sp_route(*geom, world, exchange, mx, att, mx and opt.get("fused", True),
                                       opt.get("mx_return", True), opt.get("split", True))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"S{c[0][2]}-w{c[1]}-{c[2]}-{'mx' if c[3] else 'bf'}-{'amx' if c[4] else 'abf'}"
                                                      + "".join(f"-{k}{int(v)}" for k, v in c[5].items()))
def test_route_is_what_the_gpu_tests_assert(pkg, case):
    r = _route(pkg, case)
    p = r.path()
    assert (p["layout"], p["return"], p["attention"]) == case[6] and set(p) == {"layout", "return", "attention"}, (r, p)
    assert r.amx == (p["attention"] == "mxfp8") and r.mx_return == (p["return"] == "e4m3")


def test_clip_returns_in_two_parts(pkg):
    """18 432 tokens on 2 ranks: a whole round + a split-KV tail, so the first launch completes at least one token band and that
    band goes home under the tail; with _split_return off the return is one collective."""
    for mx in (False, True):
        r = _route(pkg, (CLIP, 2, "a2a", mx, False, {}, None))
        assert list(r.launches) == pkg.native.attention_plan(1, 4, 18432, 18432) and len(r.launches) == 2
        assert r.first_bands >= 1 and r.first_bands == r.launches[0][1] // (18432 // 2)
        assert _route(pkg, (CLIP, 2, "a2a", mx, False, {"split": False}, None)).first_bands == 0


def test_invariants_over_every_case(pkg):
    for case in CASES:
        r, world, mx = _route(pkg, case), case[1], case[3]
        assert mx or not r.mx_return, (case, r)                    # bf16 linears never give an e4m3 return
        if r.layout == "gather":
            assert not r.mx_return and r.path()["return"] == "none" and r.first_bands == 0 and not r.launches, (case, r)
        else:
            assert not r.o_mx and r.launches, (case, r)
        assert 0 <= r.first_bands <= world, (case, r)


def test_switches_are_put_back(pkg):
    Nn, lib = pkg.native, pkg.native.load_library()
    before = (lib.drn_gemm_mxfp8_force_small_m(-1), Nn.attention_mxfp8_force(-1), lib.drn_gemm_tile_choice(2048, 2048))
    _route(pkg, CASES[0])
    _route(pkg, (WIDE, 2, "a2a", True, True, {}, None))
    assert (lib.drn_gemm_mxfp8_force_small_m(-1), Nn.attention_mxfp8_force(-1), lib.drn_gemm_tile_choice(2048, 2048)) == before
