"""DPM-Solver++(2M) sampler: the reference of drn_sampler_step_2m (sampler.step_reference) written out in numpy on raw bf16 bits,
independently of sampler.py; the case grid of tests/test_sampler_gpu.py; the wrong stand-ins that tests/test_sampler_cpu.py shows
the grid to separate; and the analytic Gaussian denoiser of the order-of-convergence tests.

bf16 tensors are uint16 arrays of their bits, the history is float32; all arithmetic is numpy float32, one rounding per operation.
A coefficient record is anything with sampler.Step's fields (the tests hand over the planner's own records: the planner is checked
on its own against formulas restated in test_sampler_cpu.py)."""
import zlib

import numpy as np

from latent_tile_refs import bf16_bits, f32, grid_values, rbf

# what a wrong kernel (or a wrong loop around a right one) could do instead; step_ref(..., variant=name)
VARIANTS = ("hist_not_updated", "hist_is_m", "hist_is_x", "b_swapped", "hist_read_on_first", "last_not_first_order", "cfg_on_D",
            "scaled_current_c_in", "one_copy", "fma_D1", "fma_D2", "fma_s1", "fma_s2", "fma_x", "cfg_fma", "scaled_unrounded")

SIZES = (1, 7, 8, 255, 256, 257)
SWEEP = 2048 * 256 * 8                          # one sweep of the capped grid on the 8-per-lane path
BIG = (SWEEP + 2051, SWEEP + 2048)              # past one sweep, with a tail; and one whose second copy stays 16-byte aligned
SLOTS = ("cond", "uncond", "x", "hist_in", "hist_out", "x_out", "scaled_out")
GUIDANCE = 1.5
PLAN_STEPS = 8
KINDS = {"first": 0, "middle": 3, "last": 7}    # indices into the 8-step plan


def fma(a, b, c):
    """float32(a * b + c) with the product unrounded (exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def step_ref(c, u, g, x, h, coef, copies, prior=None, variant=None):
    """c (and u, or None for no CFG) and x bits [n], h float32 [n] or None, coef a Step, prior what the hist_out buffer held before
    the call (the stand-ins that read or keep it need it) -> (x_out bits [n], hist_out float32 [n], scaled bits [copies, n] or None).
      m = u is None ? c : bf16(c + bf16(g * bf16(c - u)));  D = c_skip * x + c_out * m;  s = b1 * D (+ b0 * h where has_hist)
      x_out = bf16(a * x + s);  hist_out = D;  scaled = bf16(fp32(x_out) * c_in_next), `copies` times, absent on the last step."""
    F = np.float32
    c_skip, c_out, a, b1, b0, g = (F(v) for v in (coef.c_skip, coef.c_out, coef.a, coef.b1, coef.b0, g))
    has_hist, last = bool(coef.has_hist), coef.c_in_next is None
    if variant == "b_swapped":
        b0, b1 = b1, b0
    if variant == "hist_read_on_first" and not has_hist:
        has_hist, h = True, prior
    if variant == "last_not_first_order" and last:
        has_hist, h, b1, b0 = True, prior, F(1.5), F(-0.5)
    with np.errstate(all="ignore"):
        cf, xf = f32(c), f32(x)

        def den(mm):
            if variant == "fma_D1":
                return fma(c_skip, xf, c_out * mm)
            if variant == "fma_D2":
                return fma(c_out, mm, c_skip * xf)
            return c_skip * xf + c_out * mm
        if u is None or variant == "cfg_on_D":
            m = cf
        elif variant == "cfg_fma":
            m = rbf(fma(g, rbf(cf - f32(u)), cf))
        else:
            m = rbf(cf + rbf(g * rbf(cf - f32(u))))
        D = den(m)
        if variant == "cfg_on_D" and u is not None:             # the two halves denoised, then combined in fp32
            Du = den(f32(u))
            D = D + g * (D - Du)
        s = b1 * D
        if has_hist:
            hh = np.asarray(h, F)
            if variant == "fma_s1":
                s = fma(b0, hh, s)
            elif variant == "fma_s2":
                s = fma(b1, D, b0 * hh)
            else:
                s = s + b0 * hh
        v = fma(a, xf, s) if variant == "fma_x" else a * xf + s
        assert v.dtype == F and D.dtype == F
        xo = bf16_bits(v)
        hist_out = {"hist_not_updated": prior, "hist_is_m": m, "hist_is_x": xf}.get(variant, D)
        scaled = None
        if not last:
            src = v if variant == "scaled_unrounded" else f32(xo)
            cn = F(coef.c_in if variant == "scaled_current_c_in" else coef.c_in_next)
            one = bf16_bits(src * cn)
            scaled = np.stack([one] * copies)
            if variant == "one_copy" and copies == 2:
                scaled[1] = 0
    return xo, np.array(hist_out, dtype=F), scaled


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def case_inputs(name, n, coef, cfg):
    """Deterministic inputs of a case -> c, u (or None), x bits and h, prior float32: network outputs of scale 1, a latent of the
    step's noise level (1 / c_in = sqrt(sigma^2 + sigma_data^2)), a history of scale 1 with full fp32 mantissas."""
    r = _rng(name)
    c = bf16_bits(r.standard_normal(n).astype(np.float32))
    u = bf16_bits(r.standard_normal(n).astype(np.float32)) if cfg else None
    x = bf16_bits((r.standard_normal(n) / coef.c_in).astype(np.float32))
    h = r.standard_normal(n).astype(np.float32)
    prior = r.standard_normal(n).astype(np.float32)
    return c, u, x, h, prior


def all_finite_bf16():
    """Every finite bf16 value: 65 280 bit patterns (both zeros, the denormals, up to +-3.39e38)."""
    pos = np.arange(0, 0x7F80, dtype=np.uint32)
    return np.concatenate([pos, pos | 0x8000]).astype(np.uint16)


def value_grid(coef, cfg):
    """Every finite bf16 value of x, twice -> c, u (or None), x bits, h float32 [130 560].  First half: network outputs that walk
    through every bf16 in [-4, 4], a random history.  Second half, structured so that a contracted multiply-add is seen in the
    bf16 latent: where the step reads a history, h = -(a x + b1 D) / b0 rounded to fp32, so that the three terms of a x + b1 D +
    b0 h cancel to the last bits and what is left is the roundings of the products; where it reads none, the network output
    nearest to the one that makes b1 D cancel a x (8 bits of cancellation: one element in a few hundred then sits on a bf16 tie's
    edge).  Values that would overflow fall back to the first half's."""
    F = np.float32
    x1 = all_finite_bf16()
    n = x1.size
    g = grid_values()
    r = _rng("sampler.grid")
    c1 = g[(np.arange(n) * 7) % g.size]
    u1 = g[(np.arange(n) * 13 + 5) % g.size] if cfg else None
    h1 = r.standard_normal(n).astype(F)
    c2, h2 = c1.copy(), r.standard_normal(n).astype(F)
    xf = f32(x1).astype(np.float64)
    with np.errstate(all="ignore"):
        if not coef.has_hist and coef.b1 != 0.0 and not cfg:
            want = (-(coef.a / coef.b1) * xf - coef.c_skip * xf) / coef.c_out
            ok = np.isfinite(want) & (np.abs(want) < 1e30)
            c2 = np.where(ok, bf16_bits(np.where(ok, want, 0.0).astype(F)), c1)
        if coef.has_hist:
            _, D, _ = step_ref(c2, u1, GUIDANCE, x1, h2, coef, 1)
            want = -(float(coef.a) * xf + float(coef.b1) * D.astype(np.float64)) / float(coef.b0)
            ok = np.isfinite(want) & (np.abs(want) < 1e30)
            h2 = np.where(ok, np.where(ok, want, 0.0).astype(F), h2)
    cat = np.concatenate
    return cat([c1, c2]), (cat([u1, u1]) if cfg else None), cat([x1, x1]), cat([h1, h2])


def kernel_cases():
    """(name, n, offsets by slot, cfg, copies, kind, alias) of the geometry grid: every small size, every tensor in turn at element
    offsets 0..7 (offset 0 everywhere: the 8-per-lane path, wherever the second copy stays aligned; any other: one element per
    lane); CFG, copies, the step's kind and the aliasing of the history alternate with the case's number, and a tensor that is
    moved is always one the launch uses."""
    cases, k = [], 0
    for n in SIZES:
        for slot in SLOTS:
            for off in range(8):
                k += 1
                j = k + k // 8 + k // 56                 # (the offsets have period 8, the slots 56: the flags must not keep step)
                cfg, copies, kind, alias = bool(j % 2), 1 + (j // 2) % 2, ("first", "middle", "last")[j % 3], bool((j // 3) % 2)
                if slot == "uncond":
                    cfg = True
                if slot == "hist_in":
                    kind = "middle"
                if slot == "scaled_out" and kind == "last":
                    kind = "first"
                if slot in ("hist_in", "hist_out") and off:
                    alias = False                        # two different offsets for one buffer: two buffers
                offs = {s: 0 for s in SLOTS}
                offs[slot] = off
                cases.append((f"{n}.{slot}+{off}", n, offs, cfg, copies, kind, alias and kind == "middle"))
    zero = {s: 0 for s in SLOTS}
    cases.append((f"big.tail", BIG[0], dict(zero), True, 1, "middle", True))
    cases.append((f"big.tail.scalar", BIG[0], dict(zero, x=3), False, 2, "first", False))
    cases.append((f"big.copies", BIG[1], dict(zero), True, 2, "middle", False))
    cases.append((f"big.last", BIG[1], dict(zero), False, 1, "last", False))
    return cases


# ----------------------------------------------------------------------------------------------- order of convergence
SIGMA_MAX, SIGMA_MIN, SIGMA_DATA = 80.0, 0.02, 0.5


def gaussian_problem():
    """x0 = randn(16, 4096, float64, seed 0) * 80 and the data's standard deviation per row, linspace(0.2, 1.0, 16)[:, None]."""
    import torch
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(16, 4096, dtype=torch.float64, generator=g) * SIGMA_MAX
    return x0, torch.linspace(0.2, 1.0, 16, dtype=torch.float64)[:, None]


def gaussian_denoiser(x, sigma, std):
    """E[data | x] for data ~ N(0, std^2) seen through noise of `sigma`."""
    return x * (std ** 2 / (std ** 2 + sigma ** 2))


def gaussian_truth(x0, std):
    """The exact solution of the probability-flow ODE from sigma_max down to sigma_min, then the denoiser at sigma_min."""
    x = x0 * ((std ** 2 + SIGMA_MIN ** 2) / (std ** 2 + SIGMA_MAX ** 2)).sqrt()
    return gaussian_denoiser(x, SIGMA_MIN, std)
