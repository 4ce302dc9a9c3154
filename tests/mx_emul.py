"""Torch emulation of the MXFP8 format of include/drn.h (OCP MX v1.0: e4m3fn elements, one E8M0 scale per 32 elements along K)
and of the fp32 oracle with MXFP8 block linears.  Used by tests/test_mxfp8_*.py; nothing here runs on the GPU."""
import torch
import torch.nn.functional as F

E4M3_MAX = 448.0


def block_exponents(x: torch.Tensor) -> torch.Tensor:
    """[rows, K] (bf16 values, any float dtype) -> int32 [rows, K / 32]: floor(log2(amax)) - 8, + 1 when amax / 2^e > 448,
    clamped to [-127, 127]; -127 for an all-zero block."""
    rows, K = x.shape
    assert K % 32 == 0
    amax = x.float().abs().view(rows, K // 32, 32).amax(-1)
    mant, ex = torch.frexp(amax)                                     # amax = mant * 2^ex, mant in [0.5, 1)
    e = (ex.to(torch.int32) - 1) - 8                                 # floor(log2(amax)) - 8
    e = torch.where(mant * 2 > 1.75, e + 1, e)                        # amax / 2^e > 448
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp(-127, 127)
    return e.to(torch.int32)


def pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float32 from the bit pattern, e in [-126, 127]."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quantize(x: torch.Tensor):
    """[rows, K] -> (q [rows, K] float8_e4m3fn, scales [rows, K / 32] uint8 = e + 127): q = rne_e4m3fn(x / 2^e)."""
    rows, K = x.shape
    e = block_exponents(x)
    xs = x.float().view(rows, K // 32, 32) * pow2(-e).unsqueeze(-1)       # exact: a power of two, -e in [-127, 127]
    q = xs.view(rows, K).to(torch.float8_e4m3fn)
    return q, (e + 127).to(torch.uint8)


def dequantize(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    rows, K = q.shape
    e = scales.to(torch.int32) - 127
    return torch.ldexp(q.float().view(rows, K // 32, 32), e.unsqueeze(-1).float()).view(rows, K)


def qdq(x: torch.Tensor) -> torch.Tensor:
    """quantise -> dequantise, in x's dtype."""
    return dequantize(*quantize(x.reshape(-1, x.shape[-1]))).view(x.shape).to(x.dtype)


def mx_linear(x, w):
    return F.linear(qdq(x), qdq(w))


def mx_oracle(base_cls):
    """A subclass of oracle.dit_oracle.DitOracle whose block linears (self-attention q / k / v / out, MLP layer1 / layer2) run on
    MXFP8 quantise -> dequantise operands; the cross-attention, AdaLN, patch-embed and final linears stay as they are."""
    from oracle import dit_oracle as O

    class MxDitOracle(base_cls):
        def attention(self, pre, x, context, cos, sin):
            if context is not None:
                return super().attention(pre, x, context, cos, sin)
            q = mx_linear(x, self.w(pre + "to_q.0.weight"))
            k = mx_linear(x, self.w(pre + "to_k.0.weight"))
            v = mx_linear(x, self.w(pre + "to_v.0.weight"))
            q = q.reshape(q.shape[0], q.shape[1], self.Hn, self.dh)
            k = k.reshape(k.shape[0], k.shape[1], self.Hn, self.dh)
            v = v.reshape(v.shape[0], v.shape[1], self.Hn, self.dh)
            q = O.rms_norm(q, self.w(pre + "to_q.1.weight"))
            k = O.rms_norm(k, self.w(pre + "to_k.1.weight"))
            if cos is not None:
                q = O.apply_rope(q, cos, sin)
                k = O.apply_rope(k, cos, sin)
            o = F.scaled_dot_product_attention(q.permute(1, 2, 0, 3), k.permute(1, 2, 0, 3), v.permute(1, 2, 0, 3))
            o = o.permute(2, 0, 1, 3)
            o = o.reshape(o.shape[0], o.shape[1], -1)
            return mx_linear(o, self.w(pre + "to_out.0.weight"))

        def mlp(self, pre, x):
            return mx_linear(F.gelu(mx_linear(x, self.w(pre + "layer1.weight"))), self.w(pre + "layer2.weight"))

    return MxDitOracle
