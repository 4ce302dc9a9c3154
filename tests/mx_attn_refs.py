"""References, emulation, exact-data builders and mutated stand-ins for the MXFP8 self-attention (include/drn.h, csrc/attention_mx.hip).
Used by tests/test_mx_attn_refs_cpu.py (the proof that the bounds pass a correct emulation and fail wrong ones) and by
tests/test_mx_attn_gpu.py.  Nothing here runs on the GPU.  Layouts are those of drn.h:
  Q, K : elements [rows, H*128] e4m3 + scales [rows, H*4]      (mx_emul.quantize on the rows: 32-blocks along the head dim)
  V    : VT [B, H, 128, Skp] e4m3 + VS [B, H, 128, Skp/32]     (mx_emul.quantize on V^T zero-padded to Skp = Sk rounded up to 128)"""
import math
from collections import namedtuple

import torch

import mx_emul as MX

BF = torch.bfloat16
F64 = torch.float64
LOG2E = 1.44269504088896340736

# the bounds the GPU tests assert (test_mx_attn_gpu.py section 3; the issue's figures, reasoned there)
REL_MARGIN = 1.25          # e_hip <= 1.25 e_emul: this project's margin for HIP against an MX emulation (fp32 summation order, v_exp_f32)
ABS_FRACTION = 0.14        # max|O - O_exact| <= 0.14 max|V|: 2 * 2^-4 / (1 - 2^-4), a 2^-4 relative error on every p
EMUL_ABS_CEILING = 0.018   # what the correct emulation stays under on the grid inputs (checked on the CPU)

# the random-data grid: Sq x Sk x B x logit std x {unsplit, split}
Case = namedtuple("Case", "Sq Sk B std ns")
GRID = [Case(Sq, Sk, B, std, ns) for Sq in (16, 256, 300) for Sk in (128, 200, 768) for B in (1, 2) for std in (1, 4, 12)
        for ns in (1, 2)]
HEADS = 2
MUTANTS = ("v_scale_neighbour", "drop_key", "unmasked_tail", "p_scale_x2", "clip0_kv", "pv_order_one_side")


def case_id(c):
    return f"Sq{c.Sq}-Sk{c.Sk}-B{c.B}-std{c.std}-ns{c.ns}"


def pad128(n):
    return (n + 127) // 128 * 128


# ------------------------------------------------------------------------------------------------ quantisers
def quantize_rows(x):
    """[rows, H*128] bf16 -> (q e4m3, scales uint8): the Q / K layout."""
    return MX.quantize(x)


def quantize_vt(v, heads):
    """v [B, Sk, H*128] bf16 -> (vt [B, H, 128, Skp] e4m3, vs [B, H, 128, Skp/32] uint8): mx_emul.quantize on V^T, keys padded with
    zeros to Skp (an all-zero block gets scale byte 0)."""
    B, Sk, HD = v.shape
    Skp = pad128(Sk)
    t = torch.zeros((B, heads, 128, Skp), dtype=v.dtype)
    t[..., :Sk] = v.view(B, Sk, heads, 128).permute(0, 2, 3, 1)
    q, s = MX.quantize(t.view(-1, Skp))
    return q.view(B, heads, 128, Skp), s.view(B, heads, 128, Skp // 32)


def dequant_rows(q, s):
    return MX.dequantize(q, s)


def dequant_vt(vt, vs, Sk):
    """-> V [B, Sk, H*128] float32 (the padded keys dropped)."""
    B, H, _, Skp = vt.shape
    d = MX.dequantize(vt.reshape(-1, Skp), vs.reshape(-1, Skp // 32)).view(B, H, 128, Skp)
    return d[..., :Sk].permute(0, 3, 1, 2).reshape(B, Sk, H * 128)


# ------------------------------------------------------------------------------------------------ fp64 reference
def attention_exact(qd, kd, vd, heads, scale=None):
    """Exact (fp64) non-causal attention of the DEQUANTISED operands: qd [B, Sq, H*128], kd / vd [B, Sk, H*128] -> [B, Sq, H*128]."""
    scale = 1.0 / math.sqrt(128) if scale is None else scale
    B, Sq, HD = qd.shape
    q = qd.to(F64).view(B, Sq, heads, 128).transpose(1, 2)
    k = kd.to(F64).view(B, -1, heads, 128).transpose(1, 2)
    v = vd.to(F64).view(B, -1, heads, 128).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    return (p @ v).transpose(1, 2).reshape(B, Sq, HD)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic
def tile_key_order():
    """MFMA row order of a 128-key tile: entry 16 t + m is the key that row m of MFMA t reads (attention_mx.hip)."""
    return torch.tensor([(0 if t < 4 else 64) + 16 * (m >> 2) + 4 * (t & 3) + (m & 3) for t in range(8) for m in range(16)])


def kv_chunks(Sk, ns, key_tile):
    """The key chunks of a split launch: (begin, end) pairs; chunk = ceil(Sk / ns) rounded up to the key tile, no empty chunk."""
    if ns <= 1:
        return [(0, Sk)]
    chunk = ((Sk + ns - 1) // ns + key_tile - 1) // key_tile * key_tile
    return [(b, min(b + chunk, Sk)) for b in range(0, Sk, chunk)]


def attention_emul(qq, qs, kq, ks, vt, vs, B, Sq, Sk, policy, scale=None, ns=1, mutant=None, q_bs=None, k_bs=None):
    """The kernel's arithmetic in torch: per key tile the fp32 scores of the dequantised q and k times scale*log2(e), the lazily
    rescaled reference maximum (`policy` = (key_tile, rescale_thr, pexp) as drn_attention_mxfp8_params reports), P = rne_e4m3(p 2^pexp)
    under the operand scale 2^-pexp, the denominator summed from the quantised P, bf16 output; ns > 1: per-chunk partials merged
    as the combine pass does.  -> [B, Sq, H*128] bf16.  `mutant`: one of MUTANTS (a subtly wrong kernel)."""
    key_tile, thr, pexp = policy
    scale = 1.0 / math.sqrt(128) if scale is None else scale
    c = torch.tensor(scale * LOG2E, dtype=torch.float32)
    thr_raw = torch.tensor(float(thr), dtype=torch.float32) / c
    H = qq.shape[1] // 128
    q_bs = Sq if q_bs is None else q_bs
    k_bs = Sk if k_bs is None else k_bs
    Skp = vt.shape[-1]
    qd = dequant_rows(qq, qs)
    kd = dequant_rows(kq, ks)
    vsm = vs
    if mutant == "v_scale_neighbour":                  # the scale of the neighbouring 32-key block
        vsm = torch.roll(vs, 1, -1)
    vd = MX.dequantize(vt.reshape(-1, Skp), vsm.reshape(-1, Skp // 32)).view(B, H, 128, Skp).transpose(-1, -2)    # [B, H, Skp, 128]
    q = torch.stack([qd[b * q_bs:b * q_bs + Sq] for b in range(B)]).view(B, Sq, H, 128).transpose(1, 2)        # [B, H, Sq, 128]
    k = torch.stack([kd[b * k_bs:b * k_bs + Sk] for b in range(B)]).view(B, Sk, H, 128).transpose(1, 2)
    if mutant == "clip0_kv" and B > 1:                 # every clip attends to clip 0's keys and values
        k = k[:1].expand(B, -1, -1, -1)
        vd = vd[:1].expand(B, -1, -1, -1)
    order = tile_key_order()
    pscale = 2.0 ** -pexp
    parts = []
    for cb, ce in kv_chunks(Sk, ns, key_tile):
        m = torch.full((B, H, Sq), -math.inf)
        l = torch.zeros((B, H, Sq))
        acc = torch.zeros((B, H, Sq, 128))
        for t0 in range(cb, ce, key_tile):
            t1 = min(t0 + key_tile, ce)
            s = q @ k[:, :, t0:t1].transpose(-1, -2)                       # fp32 accumulate of dequant(q) . dequant(k)
            vtile = vd[:, :, t0:t0 + key_tile]
            if t1 - t0 < key_tile:
                # the tile's tail: the K rows are clamped to the last key (what the staging reads), the scores masked
                tail = (q @ k[:, :, t1 - 1:t1].transpose(-1, -2)).expand(-1, -1, -1, key_tile - (t1 - t0))
                s = torch.cat([s, tail if mutant == "unmasked_tail" else torch.full_like(tail, -math.inf)], -1)
            if mutant == "drop_key" and t0 <= (cb + ce) // 2 < t1:
                s[..., (cb + ce) // 2 - t0] = -math.inf
            mx = s.amax(-1)
            up = mx > m + thr_raw
            m_new = torch.where(up, mx, m)
            alpha = torch.where(up, torch.exp2((m - m_new) * c), torch.ones_like(m))
            m = m_new
            l = l * alpha
            acc = acc * alpha.unsqueeze(-1)
            p8 = torch.exp2(s * c - (m * c - pexp).unsqueeze(-1)).to(torch.float8_e4m3fn).float()        # rne_e4m3(p 2^pexp)
            l = l + p8.sum(-1) * pscale
            pv = p8[..., order] if mutant == "pv_order_one_side" else p8                                   # P in MFMA row order, V natural
            acc = acc + (pv @ vtile) * (2 * pscale if mutant == "p_scale_x2" else pscale)
        parts.append((m, l, acc))
    if len(parts) == 1:
        m, l, acc = parts[0]
        o = acc / l.unsqueeze(-1)
    else:
        mmax = torch.stack([p[0] for p in parts]).amax(0)
        den = torch.zeros_like(mmax)
        num = torch.zeros_like(parts[0][2])
        for m, l, acc in parts:
            w = torch.exp2((m - mmax) * c)
            den = den + w * l
            num = num + w.unsqueeze(-1) * acc
        o = num / den.unsqueeze(-1)
    return o.transpose(1, 2).reshape(B, Sq, H * 128).to(BF)


# ------------------------------------------------------------------------------------------------ inputs
def random_case(c, heads=HEADS, seed=None):
    """bf16 q [B*Sq, HD] (entries N(0, std^2): logit std = c.std), k [B*Sk, HD] and v [B, Sk, HD] (unit variance), quantised.
    -> dict of the MX operands and their dequantised forms."""
    seed = c.Sq * 7 + c.Sk * 3 + c.B * 1000 + c.std * 17 + c.ns if seed is None else seed
    g = torch.Generator(device="cpu").manual_seed(seed)
    HD = heads * 128
    q = (torch.randn((c.B * c.Sq, HD), generator=g) * c.std).to(BF)
    k = torch.randn((c.B * c.Sk, HD), generator=g).to(BF)
    v = torch.randn((c.B, c.Sk, HD), generator=g).to(BF)
    return operands(q, k, v, c.B, c.Sq, c.Sk, heads)


def operands(q, k, v, B, Sq, Sk, heads):
    qq, qs = quantize_rows(q)
    kq, ks = quantize_rows(k)
    vt, vs = quantize_vt(v, heads)
    qd = dequant_rows(qq, qs).view(B, Sq, -1)
    kd = dequant_rows(kq, ks).view(B, Sk, -1)
    vd = dequant_vt(vt, vs, Sk)
    return dict(qq=qq, qs=qs, kq=kq, ks=ks, vt=vt, vs=vs, qd=qd, kd=kd, vd=vd, exact=attention_exact(qd, kd, vd, heads))


def check_bounds(out, ops, e_emul):
    """The two bounds of the random-data test: -> (ok, e, worst / max|V|)."""
    from conftest import rel_l2
    e = rel_l2(out.float(), ops["exact"])
    worst = (out.double() - ops["exact"]).abs().max().item() / ops["vd"].abs().max().item()
    return (e <= REL_MARGIN * e_emul and worst <= ABS_FRACTION), e, worst


def spike_case(Sq=300, Sk=384, heads=HEADS, seed=1):
    """K rows are random +-16 vectors (exact in MXFP8), query i is the K row of key pi(i): its score beats every other by a wide
    gap, so P is exactly one-hot and output row i must be the dequantised V row pi(i), bit for bit.  -> (ops, pi, want bf16)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    HD = heads * 128
    k = (torch.randint(0, 2, (Sk, HD), generator=g).float() * 32 - 16).to(BF)
    pi = (torch.arange(Sq) * 131 + 7) % Sk
    q = k[pi].clone()
    v = torch.randn((1, Sk, HD), generator=g).to(BF)
    ops = operands(q, k, v, 1, Sq, Sk, heads)
    want = ops["vd"][0][pi].to(BF).unsqueeze(0)
    return ops, pi, want


def spike_gap(ops, pi, heads=HEADS):
    """Smallest margin, in log2 units, between a query's matching key and its best other key."""
    c = LOG2E / math.sqrt(128)
    Sq = pi.numel()
    q = ops["qd"][0].view(Sq, heads, 128).transpose(0, 1).double()
    k = ops["kd"][0].view(-1, heads, 128).transpose(0, 1).double()
    s = q @ k.transpose(-1, -2) * c
    hit = s.gather(-1, pi.view(1, Sq, 1).expand(heads, Sq, 1)).squeeze(-1)
    s.scatter_(-1, pi.view(1, Sq, 1).expand(heads, Sq, 1), -math.inf)
    return (hit - s.amax(-1)).min().item()


def uniform_case(Sq=300, Sk=200, heads=HEADS, seed=2):
    """Q = 0 makes every p exactly 1; V is small integers times per-block powers of two (exact in MXFP8), so the output is
    sum(V) / Sk: within 1 bf16 ulp of that.  -> (ops, ref float64 [1, Sq, HD])."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    HD = heads * 128
    Skp = pad128(Sk)
    q = torch.zeros((Sq, HD), dtype=BF)
    k = torch.randn((Sk, HD), generator=g).to(BF)
    ints = torch.randint(-7, 8, (heads, 128, Skp), generator=g).float()
    ints.view(heads, 128, Skp // 32, 32)[..., 0] = 7.0                    # every block's maximum is 7: its scale is the chosen power of two
    pw = torch.randint(-2, 3, (heads, 128, Skp // 32, 1), generator=g).float()
    vt = (ints.view(heads, 128, Skp // 32, 32) * torch.exp2(pw)).view(heads, 128, Skp)[..., :Sk]
    v = vt.permute(2, 0, 1).reshape(1, Sk, HD).to(BF)
    ops = operands(q, k, v, 1, Sq, Sk, heads)
    assert torch.equal(ops["vd"], v.float()), "V must be exact in MXFP8"
    ref = v.double().mean(1, keepdim=True).expand(1, Sq, HD)
    return ops, ref


# ------------------------------------------------------------------------------------------------ model level
def mx_attn_oracle(base_cls, policy, heads):
    """A subclass of an oracle class whose SELF-attention core is the emulation above: q and k after norm + RoPE and v are rounded
    to bf16 (where the kernels round) and quantised, the attention is attention_emul under `policy`."""
    from oracle import dit_oracle as O

    class MxAttnOracle(base_cls):
        def attention(self, pre, x, context, cos, sin):
            if context is not None:
                return super().attention(pre, x, context, cos, sin)
            lin = self._mx_attn_linear
            q = lin(x, self.w(pre + "to_q.0.weight"))
            k = lin(x, self.w(pre + "to_k.0.weight"))
            v = lin(x, self.w(pre + "to_v.0.weight"))
            S, B = q.shape[0], q.shape[1]
            q = O.rms_norm(q.reshape(S, B, self.Hn, self.dh), self.w(pre + "to_q.1.weight"))
            k = O.rms_norm(k.reshape(S, B, self.Hn, self.dh), self.w(pre + "to_k.1.weight"))
            if cos is not None:
                q = O.apply_rope(q, cos, sin)
                k = O.apply_rope(k, cos, sin)
            qb = q.permute(1, 0, 2, 3).reshape(B * S, -1).to(BF)
            kb = k.permute(1, 0, 2, 3).reshape(B * S, -1).to(BF)
            vb = v.permute(1, 0, 2).reshape(B, S, -1).to(BF)
            qq, qs = quantize_rows(qb)
            kq, ks = quantize_rows(kb)
            vt, vs = quantize_vt(vb, self.Hn)
            o = attention_emul(qq, qs, kq, ks, vt, vs, B, S, S, policy)                       # [B, S, HD] bf16
            o = o.to(x.dtype).permute(1, 0, 2)
            return lin(o, self.w(pre + "to_out.0.weight"))

        @staticmethod
        def _mx_attn_linear(x, w):
            return torch.nn.functional.linear(x, w)

    return MxAttnOracle


def mx_attn_mx_linear_oracle(base_cls, policy, heads):
    """The same with the block linears on MXFP8 operands (mx_emul.mx_oracle's linears)."""
    cls = mx_attn_oracle(MX.mx_oracle(base_cls), policy, heads)
    cls._mx_attn_linear = staticmethod(MX.mx_linear)
    return cls
