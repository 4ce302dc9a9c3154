"""Step cache: reuse the DiT's tail across neighbouring denoising steps, probed behind the first block.

Neighbouring steps of a sampler often leave almost the same hidden states, most of all late in the schedule.  A forward is cut in
three: the HEAD (patch embed + block 0; `X1` is the residual stream behind it, complete), the TAIL (blocks 1 .. L-1; `X_end`) and
the FINAL layer (LayerNorm + projection + unpatchify).  Per sample loop of `n` steps, with a threshold `thr` > 0 and `max_run`:

  computed step   head; ref <- X1 (a copy); tail; R <- bf16(fp32(X_end) - fp32(ref)); final.  `ref` and `R` are kept.
  candidate step  head; per clip b of the batch, over its values in memory order: num_b = sum |x_i - ref_i| (the subtraction one
                  rounded fp32 operation), den_b = sum |ref_i|, both in fp64; delta_b = num_b / den_b in host float64, with
                  den_b == 0 or anything non-finite counting as +inf; delta = max_b delta_b.  Skipped iff delta < thr, else computed.
  skipped step    X <- bf16(fp32(X1) + fp32(R)) in place; final.  `ref` and `R` are NOT updated: delta measures the distance from
                  the state where R was computed, so drift accumulates by itself.

Step 0 and step n - 1 are always computed, and so is the step after `max_run` skipped steps in a row.  The decision is ONE per
forward for the whole batch (G-buffer passes x CFG halves), taken on the worst clip: the one place where a clip's bits depend on
its batch mates.  This is the first-block variant (First-Block-Cache) on purpose: TeaCache's rescaling polynomial is fitted per
model on real weights, and there are none to fit on; the probe behind block 0 needs no calibration.

`Controller` is the rule, written once over three callables and a backend of three tensor operations.  dit_engine.HipDiT drives
it with drn_dit_forward_range and the kernels of csrc/step_cache.hip; `TorchBackend` is the torch / numpy specification that CPU
devices (the tests' stand-in nets) run, with the probe's sums taken in the order include/drn.h documents, bit for bit.
"""
import logging
import math

import numpy as np
import torch

CHUNK = 8192                # values per chunk of the probe (drn.h)
MAX_RUN = 3                 # default: skipped steps in a row before a step is computed whatever the probe says

_log = logging.getLogger(__name__)


def check_step_cache(step_cache, max_run=MAX_RUN, tile_join="pixel"):
    """ValueError for a step-cache setting that cannot be honoured, from settings alone (so before any GPU work)."""
    if isinstance(step_cache, bool) or not isinstance(step_cache, (int, float, np.integer, np.floating)):
        raise ValueError(f"step_cache must be a number in [0, 1] (0 = off), got {step_cache!r}")
    if not math.isfinite(step_cache) or not 0.0 <= step_cache <= 1.0:
        raise ValueError(f"step_cache must be a finite threshold in [0, 1] (0 = off), got {step_cache!r}")
    if isinstance(max_run, bool) or not isinstance(max_run, (int, np.integer)) or max_run < 1:
        raise ValueError(f"step_cache_max_run must be an integer >= 1, got {max_run!r}")
    if step_cache > 0 and tile_join == "latent":
        raise ValueError("tile_join = 'latent' with step_cache > 0 is not implemented (every tile is a DiT call of its own per step "
                         "and would need a cache of its own): set step_cache = 0 or tile_join = 'pixel'")


def delta_from_stats(stats) -> float:
    """[(num_b, den_b), ...] as host floats -> delta = max_b num_b / den_b; den_b == 0 or anything non-finite counts as +inf."""
    worst = 0.0
    for num, den in stats:
        num, den = float(num), float(den)
        d = num / den if (den != 0.0 and math.isfinite(num) and math.isfinite(den)) else math.inf
        if not math.isfinite(d):
            d = math.inf
        worst = max(worst, d)
    return worst


# ----------------------------------------------------------------------------------------------- the specification
def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _ordered_sum(v: np.ndarray) -> float:
    """The fp64 sum of one clip's non-negative terms `v` [n] in the order of drn_step_cache_probe (include/drn.h)."""
    n = v.size
    nc = -(-n // CHUNK)
    pad = np.zeros(nc * CHUNK, dtype=np.float64)              # a lane without a value keeps 0.0, and s + 0.0 is s
    pad[:n] = v
    q = pad.reshape(nc, 4, 256, 8)                            # [chunk][trip][lane][value]: value j = trip * 2048 + lane * 8 + e
    s = np.zeros((nc, 256), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(4):
            for e in range(8):
                s = s + q[:, t, :, e]
        s = s.reshape(nc, 4, 64)
        lane = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lane ^ d]
        w = s[:, :, 0]
        part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        seg = -(-nc // 64)
        runs_in = np.zeros(64 * seg, dtype=np.float64)
        runs_in[:nc] = part
        runs_in = runs_in.reshape(64, seg)
        runs = np.zeros(64, dtype=np.float64)
        for i in range(seg):
            runs = runs + runs_in[:, i]
        total = np.float64(0.0)
        for r in runs:
            total = total + r
    return float("nan") if np.isnan(total) else float(total)


def probe_reference(x: torch.Tensor, ref: torch.Tensor) -> np.ndarray:
    """The probe's (num_b, den_b) per clip of the leading dimension -> float64 [B, 2], in the documented order (a NaN sum is the
    one quiet NaN)."""
    B = x.shape[0]
    xb, rb = _f32(_bits(x).reshape(B, -1)), _f32(_bits(ref).reshape(B, -1))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs((xb - rb).astype(np.float32)).astype(np.float64)
    a = np.abs(rb).astype(np.float64)
    return np.array([[_ordered_sum(d[b]), _ordered_sum(a[b])] for b in range(B)], dtype=np.float64).reshape(B, 2)


def _bf16(v: torch.Tensor) -> torch.Tensor:
    """.bfloat16() with every NaN as 0x7FC0 (c10's scalar rule, the kernels' rule; torch's vectorised CPU loop writes 0xFFFF)."""
    out = v.bfloat16()
    return torch.where(torch.isnan(v), torch.full_like(out, float("nan")), out)


def residual_reference(x: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    return _bf16(x.float() - ref.float())


def apply_reference(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    return _bf16(x.float() + r.float())


class TorchBackend:
    """The three tensor operations on torch tensors of any device, clips along the leading dimension (CPU devices run this)."""

    def copy(self, x, into=None):
        return x.clone() if into is None else into.copy_(x)

    def probe(self, x, ref):
        return [tuple(row) for row in probe_reference(x, ref)]

    def residual(self, x, ref, into=None):
        r = residual_reference(x, ref)
        return r if into is None else into.copy_(r)

    def apply(self, x, r):
        return x.copy_(apply_reference(x, r))


# ----------------------------------------------------------------------------------------------- the controller
class Controller:
    """One sample loop's cache.  head(inp) -> X1, tail(X1) -> X_end, final(X) -> the forward's result; each may work in place and
    return its argument.  backend: copy(x, into) -> ref, probe(x, ref) -> [(num_b, den_b)] as host numbers, residual(x_end, ref,
    into) -> R, apply(x1, R) -> X.  `log`: per step (computed, delta or None - None where the probe was not asked)."""

    def __init__(self, thr, max_run, n_steps, head, tail, final, backend):
        check_step_cache(thr, max_run)
        if not thr > 0:
            raise ValueError(f"a step cache needs a threshold > 0, got {thr!r}")
        if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
            raise ValueError(f"n_steps must be an integer >= 1, got {n_steps!r}")
        self.thr, self.max_run, self.n_steps = float(thr), int(max_run), int(n_steps)
        self.head, self.tail, self.final, self.backend = head, tail, final, backend
        self.ref = self.R = None
        self.i = self.run = 0
        self.log = []

    def step(self, inp):
        x1 = self.head(inp)
        i = self.i
        # (a forward past the announced n_steps is computed: nothing is known about what follows it)
        forced = i == 0 or i >= self.n_steps - 1 or self.run >= self.max_run or self.ref is None
        delta = None
        if not forced:
            delta = delta_from_stats(self.backend.probe(x1, self.ref))
        if not forced and delta < self.thr:
            x = self.backend.apply(x1, self.R)
            self.run += 1
            self.log.append((False, delta))
        else:
            self.ref = self.backend.copy(x1, self.ref)
            x = self.tail(x1)
            self.R = self.backend.residual(x, self.ref, self.R)
            self.run = 0
            self.log.append((True, delta))
        self.i += 1
        return self.final(x)

    def end(self):
        """Free the two buffers, write the loop's one log line -> the log."""
        self.ref = self.R = None
        _log.info("step cache (threshold %g, max_run %d): computed %d of %d steps", self.thr, self.max_run,
                  sum(1 for c, _ in self.log if c), len(self.log))
        return self.log

