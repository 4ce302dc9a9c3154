"""Shared references of the uint8 fit tests (fit.fit_frames on uint8, drn_fit_frames_u8), on top of fit_refs.py: the same case
grid with random uint8 sources, the float64 reference on `src.double() / 255`, the fp32 specification's own error against it
(E_ref), and the wrong stand-ins these inputs have to catch.  Everything here runs on the CPU; every case is computed once and
shared."""
import torch

import fit_refs as R

BF = torch.bfloat16


def source_u8(B, T, H, W, plan=None, seed=0):
    """Random bytes.  With `plan` (a scale-1 geometry): the window of frame 0 of clip 0 that the plan keeps holds every byte value
    0..255 in every channel (pixel p of the window: (p + 85 * channel) mod 256), so no byte value's conversion goes unseen."""
    g = torch.Generator().manual_seed(20251019 + seed)
    x = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    if plan is not None:
        n = plan.H_out * plan.W_out
        assert n >= 256 and plan.scale1_y and plan.scale1_x
        p = torch.arange(n).reshape(plan.H_out, plan.W_out, 1) + 85 * torch.arange(3)
        x[0, 0, plan.y0:plan.y0 + plan.H_out, plan.x0:plan.x0 + plan.W_out] = (p % 256).to(torch.uint8)
    return x


_CASES = {}


def case(pkg, gi, B, T):
    """One grid case, computed once: uint8 source, plan, the float64 reference on src / 255, the fp32 specification on
    u8_unit(src) before and after its bf16 cast, E_ref; at scale 1 also today's host chain on the kept frames."""
    key = (gi, B, T)
    if key not in _CASES:
        fit = R.fit_module(pkg)
        (H, W), mode, fh, fw = R.GEOMETRIES[gi]
        plan = fit.plan_fit(T, H, W, mode, fh, fw)
        src = source_u8(B, T, H, W, plan if gi in R.SCALE1 else None, seed=gi)
        ref64 = R.reference64(src.double() / 255, plan)
        spec32 = fit._fit_torch(fit.u8_unit(src), plan, "cpu", round_bf16=False)
        c = dict(src=src, plan=plan, ref64=ref64, spec32=spec32, e_ref=float((spec32.double() - ref64).abs().max()),
                 name=f"{R.GEOMETRY_IDS[gi]}_B{B}_T{T}", scale1=gi in R.SCALE1)
        if c["scale1"]:
            c["today"] = R.todays_ingest(kept(src.float() / 255, plan))
            assert all(int((src[0, 0, plan.y0:plan.y0 + plan.H_out, plan.x0:plan.x0 + plan.W_out, ch].reshape(-1).bincount(
                minlength=256) > 0).sum()) == 256 for ch in range(3))
        _CASES[key] = c
    return _CASES[key]


def kept(frames, plan):
    """The frames a scale-1 plan keeps: the time gather and the crop window, [B,T',H',W',3]."""
    return frames[:, plan.t_idx.long(), plan.y0:plan.y0 + plan.H_out, plan.x0:plan.x0 + plan.W_out]


# ----------------------------------------------------------------------------------------------- wrong stand-ins
def _misread(src, index_of):
    """The bytes of every frame read through another address rule: index_of(y, x, c, H, W) -> flat byte index into the frame
    (clamped into it)."""
    B, T, H, W, _ = src.shape
    y, x, c = torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(3), indexing="ij")
    idx = index_of(y, x, c, H, W).clamp(0, H * W * 3 - 1).reshape(-1)
    return src.reshape(B, T, -1)[:, :, idx].reshape(src.shape)


def wrong_stand_ins():
    """name -> f(uint8 source) -> the fp32 frames a wrong kernel would filter; through the specification each must differ in
    bits at a scale-1 case or miss the bound at some case."""
    def pitch4(y, x, c, H, W):
        return y * ((W * 3 + 3) // 4 * 4) + x * 3 + c

    def late(y, x, c, H, W):
        return (y * W + x) * 3 + c + 1

    return {
        "multiply by 1 / 255": lambda s: s.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32),
        "/ 256": lambda s: s.float() / 256.0,
        "bytes read as signed": lambda s: s.view(torch.int8).float() / 255.0,
        "channels reversed": lambda s: s.flip(-1).float() / 255.0,
        "row pitch rounded up to 4 bytes": lambda s: _misread(s, pitch4).float() / 255.0,
        "source one byte late": lambda s: _misread(s, late).float() / 255.0,
        "frame index ignored": lambda s: s[:, :1].expand_as(s).float() / 255.0,
    }


def caught(pkg, c, frames32):
    """Is the result of filtering `frames32` under the case's plan told from the right one: other bits than today's host chain at
    a scale-1 case, or outside the bound."""
    fit = R.fit_module(pkg)
    got = fit._fit_torch(frames32, c["plan"], "cpu")
    if c["scale1"] and not torch.equal(got, c["today"]):
        return True
    return not R.bound_excess(got.double(), c["ref64"], c["e_ref"])[0]
