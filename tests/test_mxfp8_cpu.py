"""MXFP8 format emulator (tests/mx_emul.py) properties and the HipDiT precision argument checks that run before any device
work (no GPU needed)."""
import pytest
import torch

import mx_emul as MX
from conftest import tiny_net


def _data():
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(64, 256, generator=g) * 2.0 ** torch.randint(-20, 20, (64, 1), generator=g).float()
    x.view(64, 8, 32)[:, 2] = 0.0
    x.view(64, 8, 32)[:9, 3] = x.view(64, 8, 32)[:9, 3].clamp(-1.0, 1.0)
    x.view(64, 8, 32)[:5, 3, 0] = 1.75 * 2.0 ** 7
    x.view(64, 8, 32)[5:9, 3, 0] = (1.75 + 2 ** -7) * 2.0 ** 7
    return x.to(torch.bfloat16)


def test_scaled_elements_never_exceed_448_and_bytes_in_range():
    x = _data()
    q, s = MX.quantize(x)
    assert torch.isfinite(q.float()).all() and q.float().abs().max() <= 448.0
    assert int(s.min()) >= 0 and int(s.max()) <= 254
    assert (s.view(64, 8)[:, 2] == 0).all()                       # all-zero block: e = -127
    # mantissa exactly 1.75 keeps floor(log2) - 8; above 1.75 takes one more
    assert (s[:5, 3].int() - 127 == 7 - 8).all() and (s[5:9, 3].int() - 127 == 7 - 8 + 1).all()


def test_representable_values_round_trip():
    g = torch.Generator(device="cpu").manual_seed(2)
    e = torch.randint(-20, 20, (32, 4), generator=g)
    codes = torch.randint(0, 256, (32, 128), generator=g).to(torch.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0x7e                              # no NaN codes
    q = codes.view(torch.float8_e4m3fn)
    q.view(torch.uint8).view(32, 4, 32)[:, :, 0] = 0x7e               # every block holds 448: its amax fixes e
    x = MX.dequantize(q, (e + 127).to(torch.uint8))
    q2, s2 = MX.quantize(x)
    assert torch.equal(s2.int() - 127, e.int())
    assert torch.equal(MX.dequantize(q2, s2), x)


def test_precision_argument_checks(pkg):
    net = tiny_net(pkg, 256, 1, 2)
    H = pkg.dit_engine.HipDiT
    with pytest.raises(ValueError, match="unknown DiT precision"):
        H(net, {}, device="cpu", precision="fp8")
    with pytest.raises(ValueError, match="not built yet"):
        H(net, {}, device="cpu", precision="mxfp8", process_group=object())
    assert pkg.dit_engine.PRECISIONS == ("bf16", "mxfp8")
