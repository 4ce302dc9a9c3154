"""CPU side of the MXFP8 self-attention tests (no GPU): the references and the emulation of tests/mx_attn_refs.py, the proof that the
bounds tests/test_mx_attn_gpu.py asserts pass the CORRECT emulation at every grid case and fail subtly wrong ones, and the
host-only C-ABI checks of the new entry points (DRN_EINVAL before any launch, sizers, policy query, struct mirror, HipDiT arguments).

What rejects which mutation (the GPU module runs the same three kinds of case):
  v_scale_neighbour, p_scale_x2, pv_order_one_side : the relative bound, at EVERY grid case (and the exact-data cases)
  clip0_kv                                          : the relative bound at every grid case with two clips
  unmasked_tail                                     : the uniform-score case (Sk = 200) and the relative bound at the Sk = 200 grid cases
                                                      with logit std <= 4 (no tail at Sk = 128, 768; at std 12 a query that has its
                                                      dominant key elsewhere hardly sees the tail)
  drop_key                                          : the spike case (pi covers every key) and the uniform-score case; on random
                                                      data one missing key of hundreds is inside the quantisation noise"""
import ctypes
import functools
import math
import os
import re

import pytest
import torch

import mx_attn_refs as R
import mx_emul as MX
from conftest import ROOT, rel_l2

BF = torch.bfloat16
POLICY = (128, 4.0, 4)          # what the library reports (test_policy_query_and_sizers holds it to that)
H = R.HEADS
NEW = ("drn_attention_mxfp8_params", "drn_qk_norm_rope_mx", "drn_mx_quant_vt", "drn_attention_mxfp8", "drn_attention_splitkv_mxfp8",
       "drn_dit_forward_mx_attn_bytes", "drn_attention_mxfp8_choice", "drn_attention_mxfp8_force")


def _emul(ops, c, mutant=None, policy=POLICY):
    return R.attention_emul(ops["qq"], ops["qs"], ops["kq"], ops["ks"], ops["vt"], ops["vs"], c.B, c.Sq, c.Sk, policy, ns=c.ns,
                            mutant=mutant)


@functools.lru_cache(maxsize=None)
def _grid_case(c):
    ops = R.random_case(c)
    return ops, rel_l2(_emul(ops, c).float(), ops["exact"])


# ------------------------------------------------------------------------------------------------ references and quantisers
def test_vt_quantiser_layout_and_padding():
    v = torch.randn((2, 200, H * 128)).to(BF)
    v[0, :32, 5] = 0
    vt, vs = R.quantize_vt(v, H)
    assert vt.shape == (2, H, 128, 256) and vs.shape == (2, H, 128, 8)
    assert int(vt.view(torch.uint8)[..., 200:].max()) == 0 and int(vs[..., 7].max()) == 0 and int(vs[0, 0, 5, 0]) == 0
    # block (b, h, d, j) is keys 32 j .. 32 j + 31 of column h * 128 + d: the same bytes as quantising that column's keys
    col = torch.zeros((1, 256))
    col[0, :200] = v[1, :, 128 + 9].float()
    q, s = MX.quantize(col.to(BF))
    assert torch.equal(q.view(torch.uint8)[0], vt.view(torch.uint8)[1, 1, 9]) and torch.equal(s[0], vs[1, 1, 9])
    assert rel_l2(R.dequant_vt(vt, vs, 200), v.float()) < 4e-2


def test_emulation_is_attention():
    """Against exact attention of the dequantised operands the emulation differs by the rounding of P alone; with the split it
    is the same arithmetic per chunk."""
    for c in (R.Case(300, 200, 2, 1, 1), R.Case(300, 768, 1, 4, 2), R.Case(16, 128, 1, 12, 1)):
        ops, e = _grid_case(c)
        assert 1e-3 < e < 4e-2, (c, e)
        plain = F_sdpa(ops, c)
        assert rel_l2(ops["exact"], plain) < 1e-5


def F_sdpa(ops, c):
    q = ops["qd"].view(c.B, c.Sq, H, 128).transpose(1, 2)
    k = ops["kd"].view(c.B, c.Sk, H, 128).transpose(1, 2)
    v = ops["vd"].view(c.B, c.Sk, H, 128).transpose(1, 2)
    return torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(c.B, c.Sq, H * 128)


def test_policy_moves_the_emulation():
    """The emulation must run under the kernel's policy: with a true running maximum (threshold 0, pexp 8) the dominant key's p
    is exactly 1 and the small ones keep more bits - a different error, which is why the GPU test reads the policy from the library."""
    c = R.Case(256, 768, 1, 4, 1)
    ops, e = _grid_case(c)
    e0 = rel_l2(_emul(ops, c, policy=(128, 0.0, 8)).float(), ops["exact"])
    assert e0 != e and 0.3 < e0 / e < 3.0, (e0, e)


# ------------------------------------------------------------------------------------------------ the bounds discriminate
@pytest.mark.parametrize("c", R.GRID, ids=R.case_id)
def test_bounds_pass_emulation_and_fail_mutants(c):
    ops, e_emul = _grid_case(c)
    ok, e, worst = R.check_bounds(_emul(ops, c), ops, e_emul)
    assert ok and worst <= R.EMUL_ABS_CEILING, (e, worst)
    fatal = ["v_scale_neighbour", "p_scale_x2", "pv_order_one_side"]
    if c.B > 1:
        fatal.append("clip0_kv")
    if c.Sk % 128 and c.std <= 4:
        fatal.append("unmasked_tail")
    for m in fatal:
        okm, em, wm = R.check_bounds(_emul(ops, c, m), ops, e_emul)
        assert not okm and em > 2 * R.REL_MARGIN * e_emul, (m, em, e_emul, wm)


def test_spike_is_one_hot_and_catches_key_mutants():
    ops, pi, want = R.spike_case()
    assert R.spike_gap(ops, pi) >= 64                                             # measured ~2400 log2 units: P is exactly one-hot
    assert len(set((pi % 128).tolist())) == 128 and set((pi // 128).tolist()) == {0, 1, 2}     # every tile position, every tile
    assert len(set(pi.tolist())) == pi.numel()
    c = lambda ns: R.Case(300, 384, 1, 0, ns)
    for ns in (1, 2, 3):
        assert torch.equal(_emul(ops, c(ns)), want), ns
        for m in ("drop_key", "v_scale_neighbour", "p_scale_x2", "pv_order_one_side"):
            assert not torch.equal(_emul(ops, c(ns), m), want), (ns, m)


def test_uniform_is_exact_and_catches_tail_and_key_mutants():
    ops, ref = R.uniform_case()

    def worst(out):
        return ((out.double() - ref).abs() / (torch.maximum(ref.abs(), out.double().abs()) * 2.0 ** -7).clamp_min(1e-30)).max().item()

    for ns in (1, 2, 3):
        c = R.Case(300, 200, 1, 0, ns)
        assert worst(_emul(ops, c)) <= 1.0
        for m in ("unmasked_tail", "drop_key", "v_scale_neighbour", "p_scale_x2", "pv_order_one_side"):
            assert worst(_emul(ops, c, m)) > 4.0, (ns, m)


def test_model_oracle_with_emulated_attention(pkg):
    """The oracle subclass of the model-level GPU test: close to the fp32 oracle, not equal to it, in both linear precisions."""
    from conftest import tiny_net
    from oracle import dit_oracle as O
    net = tiny_net(pkg, 256, 1, 2)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF)
    sw = pkg.synthetic_weights
    x = sw.synth_tensor("mxa.x", (1, 16, 2, 16, 16), torch.float32, scale=2.0).to(BF)
    cond = sw.synth_tensor("mxa.c", (1, net["additional_concat_ch"], 2, 16, 16), torch.float32).to(BF)
    t, ci = torch.tensor(2.0), torch.full((1, 1), 1, dtype=torch.long)
    with torch.no_grad():
        ref = O.DitOracle(sd, net, dtype=torch.float32, tables_dtype=BF).forward(x, t, cond, ci)
        a = R.mx_attn_oracle(O.DitOracle, POLICY, 2)(sd, net, dtype=torch.float32, tables_dtype=BF).forward(x, t, cond, ci)
        b = R.mx_attn_mx_linear_oracle(O.DitOracle, POLICY, 2)(sd, net, dtype=torch.float32, tables_dtype=BF).forward(x, t, cond, ci)
        lin = MX.mx_oracle(O.DitOracle)(sd, net, dtype=torch.float32, tables_dtype=BF).forward(x, t, cond, ci)
        a16 = R.mx_attn_oracle(O.DitOracle, POLICY, 2)(sd, net, dtype=BF).forward(x, t, cond, ci).float()
        r16 = O.DitOracle(sd, net, dtype=BF).forward(x, t, cond, ci).float()
    ea, eb, el = rel_l2(a, ref), rel_l2(b, ref), rel_l2(lin, ref)
    assert 1e-4 < ea < 0.2 and eb > el * 0.5 and eb < 0.3, (ea, eb, el)
    # in the bf16 oracle (the stand-in for an engine with bf16 linears) the emulated attention adds to the bf16 error, it does not
    # replace it: the fp32 oracle around the same attention sits BELOW the plain bf16 reference
    assert rel_l2(a16, ref) > rel_l2(r16, ref) > ea, (rel_l2(a16, ref), rel_l2(r16, ref), ea)


# ------------------------------------------------------------------------------------------------ host-only C ABI
@pytest.fixture()
def lib(pkg):
    return pkg.native.load_library()


P = 1 << 20          # a fake, aligned, never dereferenced device address


def test_new_symbols_declared_bound_and_exported(pkg, lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drn.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in pkg.native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.drn_abi_version() == 1
    assert lib.drn_dit_forward_args_bytes() == ctypes.sizeof(pkg.native.DitForwardArgs)
    names = [f[0] for f in pkg.native.DitForwardArgs._fields_]
    assert names[-4:] == ["attn_precision", "reserved2", "mx_attn", "mx_attn_bytes"]          # trailing: all-zero = today's launches
    assert pkg.dit_engine.PRECISIONS == ("bf16", "mxfp8") and pkg.dit_engine.ATTENTION_PRECISIONS == ("bf16", "mxfp8")


def test_policy_query_and_sizers(pkg, lib):
    kt, thr, pexp = pkg.native.attention_mxfp8_params()
    assert (kt, thr, pexp) == POLICY
    assert kt == 128 and 2.0 ** thr * 2.0 ** pexp <= 448                          # P stays inside e4m3 under the lazy rescale
    assert lib.drn_attention_mxfp8_params(None, None, None) == -1
    up = lambda n: (n + 255) // 256 * 256
    for B, S, Dm in ((1, 256, 4096), (2, 300, 512), (1, 18432, 4096)):
        Sp = (S + 127) // 128 * 128
        want = 2 * up(B * S * Dm) + up(B * Dm * Sp) + 2 * up(B * S * Dm // 32) + up(B * Dm * Sp // 32)
        assert lib.drn_dit_forward_mx_attn_bytes(B, S, Dm) == want
    assert lib.drn_dit_forward_mx_attn_bytes(1, 256, 4096 + 64) == 0 and lib.drn_dit_forward_mx_attn_bytes(0, 256, 4096) == 0


def test_mx_attn_layout_is_the_one_statement_of_the_scratch(pkg, lib):
    """drn_dit_forward_mx_attn_layout: the offsets HipDiT._workspace builds its views from and the sequencer reads at.  Its total is
    the sizer's, the six regions QQ | KQ | VT | QS | KS | VS follow each other 256-byte aligned without overlap (S = 300: no
    multiple of 128, so Sp != S and the regions are no multiples of 256), and it refuses where the sizer returns 0."""
    lay = (ctypes.c_int64 * 8)()
    rounded = False
    for B, S, Dm in ((1, 256, 4096), (2, 300, 512), (1, 18432, 4096)):
        assert lib.drn_dit_forward_mx_attn_layout(B, S, Dm, lay) == 0
        off, total, Sp = list(lay[:6]), lay[6], lay[7]
        assert total == lib.drn_dit_forward_mx_attn_bytes(B, S, Dm) and Sp == (S + 127) // 128 * 128
        sizes = [B * S * Dm, B * S * Dm, B * Dm * Sp, B * S * Dm // 32, B * S * Dm // 32, B * Dm * Sp // 32]
        assert off[0] == 0 and all(o % 256 == 0 for o in off)
        for i in range(6):
            end = off[i + 1] if i < 5 else total
            assert off[i] + sizes[i] <= end and end - (off[i] + sizes[i]) < 256, (B, S, Dm, i)
            rounded = rounded or end != off[i] + sizes[i]
    assert rounded                                                               # (S = 300: the scale regions are padded)
    assert lib.drn_dit_forward_mx_attn_layout(1, 256, 4096 + 64, lay) == -1 and lib.drn_dit_forward_mx_attn_layout(0, 256, 4096, lay) == -1
    assert lib.drn_dit_forward_mx_attn_layout(1, 256, 4096, None) == -1


def test_site_choice_is_a_pure_function_of_one_clips_tokens(pkg, lib):
    assert lib.drn_attention_mxfp8_force(-1) == 0
    for heads in (2, 32):
        assert [lib.drn_attention_mxfp8_choice(heads, S) for S in (1, 256, 1024, 2047, 2048, 2049, 18432)] == [0, 0, 0, 0, 1, 1, 1]
    assert lib.drn_attention_mxfp8_choice(0, 4096) == 0 and lib.drn_attention_mxfp8_choice(32, 0) == 0
    assert lib.drn_attention_mxfp8_force(1) == 0
    try:
        assert lib.drn_attention_mxfp8_choice(32, 256) == 1 and pkg.native.attention_mxfp8_choice(32, 256)
        assert lib.drn_attention_mxfp8_force(7) == 1 and lib.drn_attention_mxfp8_choice(32, 256) == 1      # a query changes nothing
    finally:
        assert lib.drn_attention_mxfp8_force(0) == 1
    assert lib.drn_attention_mxfp8_choice(32, 256) == 0


def test_producers_refuse_on_the_host(lib):
    rope, vt = lib.drn_qk_norm_rope_mx, lib.drn_mx_quant_vt

    def call(q=P, k=P, wq=P, wk=P, cos=P, sin=P, qq=P, qs=P, kq=P, ks=P, tokens=300, heads=2, ldq=768, ldk=768, tpb=150, wb=0):
        return rope(q, k, wq, wk, cos, sin, qq, qs, kq, ks, tokens, heads, ldq, ldk, tpb, 0, 1e-6, wb, None)

    assert call(q=None, k=None) == -1 and call(qq=None) == -1 and call(qs=None) == -1 and call(kq=None) == -1 and call(ks=None) == -1
    assert call(wq=None) == -1 and call(sin=None) == -1 and call(ldq=768 + 4) == -1 and call(tpb=0) == -1 and call(heads=0) == -1
    assert call(wb=2) == -1 and call(qq=P + 4) == -1 and call(q=P + 8) == -1
    assert call(tokens=0) == 0                                                    # nothing to do is not an error
    assert call(q=None, wq=None, qq=None, qs=None, tokens=0) == 0                 # k alone

    def callv(v=P, t=P, s=P, batch=2, heads=2, Sk=200, ldv=768, bsv=200 * 768):
        return vt(v, t, s, batch, heads, Sk, ldv, bsv, None)

    assert callv(v=None) == -1 and callv(t=None) == -1 and callv(s=None) == -1
    assert callv(Sk=0) == -1 and callv(batch=0) == -1 and callv(heads=0) == -1
    assert callv(ldv=128) == -1 and callv(ldv=768 + 4) == -1 and callv(bsv=200 * 768 + 4) == -1      # ldv < heads * 128, % 8
    assert callv(v=P + 8) == -1 and callv(t=P + 8) == -1 and callv(s=P + 2) == -1


def test_attention_entries_refuse_on_the_host(lib):
    one, split = lib.drn_attention_mxfp8, lib.drn_attention_splitkv_mxfp8
    Hh, S = 4, 256
    HD = Hh * 128

    def call(qq=P, qs=P, kq=P, ks=P, vt=P, vs=P, o=P, oq=None, os_=None, batch=1, heads=Hh, Sq=S, Sk=S, q_bs=S, k_bs=S, ldo=HD,
             bso=S * HD, scale=0.088, ns=None, ws=P):
        if ns is None:
            return one(qq, qs, kq, ks, vt, vs, o, oq, os_, batch, heads, Sq, Sk, q_bs, k_bs, ldo, bso, scale, None)
        return split(qq, qs, kq, ks, vt, vs, o, oq, os_, batch, heads, Sq, Sk, q_bs, k_bs, ldo, bso, scale, ns, ws, None)

    for ns in (None, 2):
        for name in ("qq", "qs", "kq", "ks", "vt", "vs"):
            assert call(ns=ns, **{name: None}) == -1, name
        assert call(ns=ns, o=None) == -1                                           # no output at all
        assert call(ns=ns, o=None, oq=P) == -1                                     # oq without os
        assert call(ns=ns, Sk=0) == -1 and call(ns=ns, heads=0) == -1 and call(ns=ns, batch=0) == -1 and call(ns=ns, scale=0.0) == -1
        assert call(ns=ns, qq=P + 8) == -1 and call(ns=ns, kq=P + 8) == -1 and call(ns=ns, vt=P + 8) == -1
        assert call(ns=ns, qs=P + 2) == -1 and call(ns=ns, ks=P + 1) == -1 and call(ns=ns, vs=P + 2) == -1
        assert call(ns=ns, ldo=HD + 4) == -1 and call(ns=ns, ldo=HD - 128) == -1 and call(ns=ns, o=P + 8) == -1
        assert call(ns=ns, batch=2, q_bs=S - 1) == -1 and call(ns=ns, batch=2, k_bs=S - 1) == -1      # clips overlap
        assert call(ns=ns, oq=P, os_=P, ldo=HD + 8) == -1                          # MX rows are contiguous
        assert call(ns=ns, oq=P, os_=P, bso=S * HD + 8) == -1 and call(ns=ns, oq=P + 4, os_=P) == -1 and call(ns=ns, oq=P, os_=P + 2) == -1
        assert call(ns=ns, Sq=0) == 0 and call(ns=ns, Sq=0, o=None, oq=P, os_=P) == 0
    assert call(ns=2, ws=None) == -1 and call(ns=2, ws=P + 8) == -1 and call(ns=0) == -1


def test_forward_refuses_mx_attention_without_scratch(pkg, lib):
    from test_mxfp8_small_m_cpu import _mx_args
    fwd = lib.drn_dit_forward

    def args(B=1, S=256, Dm=4096, hidden=16384):
        a, subs = _mx_args(pkg, lib, B, S, Dm, hidden)
        a.attn_precision, a.mx_attn = 1, P
        a.mx_attn_bytes = lib.drn_dit_forward_mx_attn_bytes(B, S, Dm)
        return a, subs

    a, subs = args()
    a.mx_attn = None
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = args()
    a.mx_attn_bytes -= 1
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = args(B=2)
    a.mx_attn_bytes = lib.drn_dit_forward_mx_attn_bytes(1, 256, 4096)           # sized for one clip, two stacked
    assert fwd(ctypes.byref(a), None) == -1
    a, subs = args()
    a.mx_attn = P + 64                                                           # the sections are 256-byte aligned
    assert fwd(ctypes.byref(a), None) == -1
    for bad in (2, -1):
        a, subs = args()
        a.attn_precision = bad
        assert fwd(ctypes.byref(a), None) == -1
    a, subs = args()                                                             # with the bf16 block linears too
    a.precision, a.mx_attn_bytes = 0, 0
    assert fwd(ctypes.byref(a), None) == -1
    # the refusals of the forward as it was are still made with the new fields present and zero
    a, subs = _mx_args(pkg, lib)
    a.AQ = None
    assert a.attn_precision == 0 and fwd(ctypes.byref(a), None) == -1


def test_hipdit_argument_checks_on_cpu(pkg, monkeypatch):
    from conftest import tiny_net
    net = tiny_net(pkg, 256, 1, 2)
    Hd = pkg.dit_engine.HipDiT
    monkeypatch.delenv("DRN_ATT_PRECISION", raising=False)
    with pytest.raises(ValueError, match="unknown attention precision"):
        Hd(net, {}, device="cpu", attention_precision="fp8")
    with pytest.raises(ValueError, match="not built yet"):
        Hd(net, {}, device="cpu", attention_precision="mxfp8", process_group=object())
    monkeypatch.setenv("DRN_ATT_PRECISION", "e4m3")
    with pytest.raises(ValueError, match="unknown attention precision"):
        Hd(net, {}, device="cpu")
    monkeypatch.setenv("DRN_ATT_PRECISION", "mxfp8")
    with pytest.raises(ValueError, match="not built yet"):
        Hd(net, {}, device="cpu", process_group=object())
    # an explicit argument wins over the environment; the engine then goes on to the weights (absent here)
    with pytest.raises(KeyError):
        Hd(net, {}, device="cpu", attention_precision="bf16")
