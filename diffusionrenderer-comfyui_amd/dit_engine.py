"""HipDiT: the CleanDiffusionRendererGeneralDIT forward on hand-written gfx950 kernels.

Host-side mirror of the reference operator `net(x, timesteps, latent_condition, context_index)`
(CleanGeneralDIT.py:731-751 -> :656-718): same call signature, same state-dict names in, same
[B,16,F,h,w] tensor out.  All arithmetic on activations runs in libdrn.so (native.py); torch is used
for device memory, tiny host tables and (multi-GPU) the RCCL all-gather.

Data layout in HBM: tokens are rows.  X [S, D] bf16 (S = F*(h/2)*(w/2) tokens in (T H W) order, the
reference's 'B T H W D -> (T H W) B D' with B = 1), QKV [S, 3D] (q | k | v, head-major 128-wide slices),
MLP hidden [S, 4D].  Weights are repacked once at load: q/k/v fused to [3D, D]; patch-embed K padded to a
multiple of 64; final projection N padded to 128; all 3*L AdaLN-LoRA down/up projections stacked for
two grouped GEMV launches per timestep.

Exact shortcuts: the cross-attention has ONE key, so softmax == 1 and its output is
to_out(to_v(context)) for every token, independent of x; its LayerNorm/modulate/q-projection are dead.
The block reduces to x += bf16(gate * c_i) with c_i cached per context index, and that broadcast add is
fused into the next sub-block's LayerNorm pass.

Sequence parallelism (one process per GPU): rank r owns a contiguous band of latent frames; every op is
token-local except self-attention.  There the ranks trade token bands for heads with one all-to-all (each rank
attends over ALL tokens of heads/world heads) and trade back afterwards; when the world size does not divide the
head count, K/V rows (after RMSNorm + RoPE) are all-gathered instead (parallel.py).  Both MXFP8 switches work under it: the
projections write / read the exchange slabs through the blocked MXFP8 GEMM, the attention output goes home as e4m3 + scales
($DRN_SP_MX_RETURN=0: as bf16), the MXFP8 attention runs on the heads a rank holds.
"""
import ctypes
import math
from typing import Dict, NamedTuple, Optional

import torch

from . import native as N
from . import step_cache as SC
from .host_tables import rope_cos_sin, timestep_sinusoid
from .parallel import ShardPlan, allgather_rows_, alltoall_bands_, alltoall_rows_, group_info, is_process_group, wait_exchange


PRECISIONS = ("bf16", "mxfp8")
ATTENTION_PRECISIONS = ("bf16", "mxfp8")


def _pad_cols(w: torch.Tensor, mult: int) -> torch.Tensor:
    n, k = w.shape
    kp = (k + mult - 1) // mult * mult
    if kp == k:
        return w.contiguous()
    out = torch.zeros((n, kp), dtype=w.dtype, device=w.device)
    out[:, :k] = w
    return out


def _pad_rows(w: torch.Tensor, mult: int) -> torch.Tensor:
    n, k = w.shape
    npad = (n + mult - 1) // mult * mult
    if npad == n:
        return w.contiguous()
    out = torch.zeros((npad, k), dtype=w.dtype, device=w.device)
    out[:n] = w
    return out


class SpRoute(NamedTuple):
    """What the self-attention blocks of one sharded forward do (sp_route)."""
    layout: str                # "gather"; a2a: "slabs" (the projections write / read the rank-major slabs) or "regroup" (GEMM + pass)
    amx: bool                  # the attention runs on the MXFP8 kernels
    mx_return: bool = False    # a2a: the attention output goes home as e4m3 + scales
    launches: tuple = ()       # a2a: native.attention_plan of the heads a rank holds
    first_bands: int = 0       # a2a: token bands launch 0 completes, sent home under launch 1 (0 = the return as one collective)
    o_mx: bool = False         # gather: O leaves the attention as MXFP8

    def path(self) -> dict:
        """HipDiT.sp_path: the route as tests and tools read it."""
        ret = "none" if self.layout == "gather" else ("e4m3" if self.mx_return else "bf16")
        return {"layout": self.layout, "return": ret, "attention": "mxfp8" if self.amx else "bf16"}


def sp_route(D, heads, S, world, exchange, mx, amx_on, fused_mx, mx_return, split_return) -> SpRoute:
    """The route of a sharded forward, from numbers and switches alone (host-only queries of native: no engine, no device).
    mx / amx_on: MXFP8 linears / attention switched on; fused_mx: the producers write MXFP8; mx_return / split_return: the
    engine's _mx_return / _split_return.  Asked once per forward, so a force switch of the library flipped in between is seen."""
    if exchange == "gather":
        amx = bool(amx_on and N.attention_mxfp8_choice(heads, S))              # per site, from ONE clip's tokens
        # fused producers: O leaves the attention as MXFP8 (the 32x32x16 body has no MX epilogue: bf16 + the quantise launch)
        return SpRoute("gather", amx, o_mx=bool(fused_mx and (amx or N.attention_mx_available())))
    W, rows, hpr = D // world, S // world, heads // world
    if mx:
        # the MXFP8 slab GEMM always runs on the 256 x 256 kernel: taken where the plan of one clip's band rows picks that
        # kernel anyway (the slab layout then changes no bit) and the planes meet its contract (drn.h)
        slabs = (world > 1 and W >= 256 and W & (W - 1) == 0
                 and N.mx_gemm_plan(rows, 2 * D, D) == 0 and N.mx_gemm_plan(rows, D, D) == 0)
    else:
        slabs = world > 1 and W >= 512 and N.gemm_blocked_ok(rows, 2 * D) and N.gemm_blocked_ok(rows, D)
    amx = bool(amx_on and N.attention_mxfp8_choice(hpr, S))
    # mxfp8: the output leaves the attention as e4m3 + scales and travels like that, where an MX epilogue exists and the receive
    # side can consume the bytes as they are: as A planes (slabs), as they lie (one rank), or through the regroup kernel over
    # byte pairs (scale rows of a multiple of 16 bytes); else bf16 goes home and is quantised there
    mxret = bool(mx and mx_return and (amx or N.attention_mx_available()) and (slabs or world == 1 or (W // 32) % 16 == 0))
    # the attention of a rank's heads is usually two launches (the q-blocks that fill whole rounds of the CUs, then the rest with
    # its keys split): the token bands whose queries the first has finished go home while the second runs
    launches = tuple(N.attention_plan(1, hpr, S, S))
    nb = launches[0][1] // rows if len(launches) == 2 and split_return else 0
    return SpRoute("slabs" if slabs else "regroup", amx, mxret, launches, nb)


class _HipCacheBackend:
    """step_cache.Controller's tensor operations on the residual stream [B S, D] (csrc/step_cache.hip); cur["B"]: its clips."""

    def __init__(self, cur):
        self.cur = cur
        self.stats = self.ws = None

    def copy(self, x, into=None):
        return x.clone() if into is None else into.copy_(x)

    def probe(self, x, ref):
        B = self.cur["B"]
        if self.stats is None:
            self.stats = torch.empty((B, 2), dtype=torch.float64, device=x.device)
            nb = N.load_library().drn_step_cache_workspace_bytes(B, x.numel() // B)
            self.ws = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
        N.step_cache_probe(x.view(B, -1), ref.view(B, -1), self.stats, self.ws)
        return self.stats.tolist()                # the step's one synchronisation: B x 2 doubles

    def residual(self, x, ref, into=None):
        return N.step_cache_residual(x, ref, out=into)

    def apply(self, x, r):
        return N.step_cache_apply(x, r)


class HipDiT:
    def __init__(self, net: dict, state_dict: Dict[str, torch.Tensor], device=None, prefix: str = "net.",
                 process_group=None, precision: Optional[str] = None, attention_precision: Optional[str] = None):
        """precision: "bf16" (default) or "mxfp8" (opt-in: the q|k|v, out-proj, MLP-up and MLP-down GEMMs of every block run on
        MXFP8 operands quantised on the device, drn.h; everything else stays bf16).  None = $DRN_DIT_PRECISION, else "bf16".
        attention_precision: "bf16" (default) or "mxfp8" (opt-in, independent of `precision`: both products of the self-attention
        run on e4m3 operands, drn.h "MXFP8 self-attention", at the sites where drn_attention_mxfp8_choice says they pay: from 2048
        tokens per clip; smaller clips keep the bf16 attention, bit for bit).  None = $DRN_ATT_PRECISION, else "bf16"."""
        import os
        if attention_precision is None:
            attention_precision = os.environ.get("DRN_ATT_PRECISION", "") or "bf16"
        if attention_precision not in ATTENTION_PRECISIONS:
            raise ValueError(f"unknown attention precision {attention_precision!r}: expected one of {ATTENTION_PRECISIONS}")
        self.attention_precision = attention_precision
        self._amx = attention_precision == "mxfp8"
        if precision is None:
            precision = os.environ.get("DRN_DIT_PRECISION", "") or "bf16"
        if precision not in PRECISIONS:
            raise ValueError(f"unknown DiT precision {precision!r}: expected one of {PRECISIONS}")
        self.precision = precision
        self._mx = precision == "mxfp8"
        # the MXFP8 exchanges carry uint8 / e4m3 payloads through torch.distributed collectives (parallel.py); a group object of
        # any other transport gets the refusal that every process group got before the sharded MXFP8 paths existed
        if (self._mx or self._amx) and process_group is not None and not is_process_group(process_group):
            which = "precision" if self._mx else "attention_precision"
            raise ValueError(f"{which}='mxfp8' with a process_group that is no torch.distributed.ProcessGroup (sequence parallelism "
                             f"over another transport) is not built yet; got {type(process_group).__name__}")
        self.net = dict(net)
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.D = net["model_channels"]
        self.heads = net["num_heads"]
        self.L = net["num_blocks"]
        self.kinds = [k.strip().lower() for k in net["block_config"].split("-")]
        self.pt, self.ps = net["patch_temporal"], net["patch_spatial"]
        self.out_ch = net["out_channels"]
        self.use_ctx = net.get("use_context_embedding", True)
        self.ctx_dim = net["crossattn_emb_channels"]
        self.with_mask = net.get("concat_padding_mask", True)
        if self.D // self.heads != 128:
            raise ValueError("HipDiT kernels are specialised for head_dim 128 (the renderer's only configuration)")
        hidden = int(self.D * net["mlp_ratio"])
        if self._mx and (self.D % 256 or hidden % 256):
            raise ValueError(f"precision='mxfp8' needs model_channels and the MLP width to be multiples of 256 (the MXFP8 GEMM's "
                             f"N and K contract); got {self.D} and {hidden}")
        N.load_library()
        self.pg = process_group
        world = group_info(process_group)[1] if process_group is not None else 1
        mode = os.environ.get("DRN_SP_EXCHANGE", "auto")
        if mode not in ("auto", "a2a", "gather"):
            raise ValueError("DRN_SP_EXCHANGE must be auto, a2a or gather")
        if mode == "a2a" and self.heads % world:
            raise ValueError(f"head all-to-all needs the world size ({world}) to divide the head count ({self.heads})")
        if process_group is None:
            self.exchange = "none"
        elif mode == "auto":
            self.exchange = "none" if world == 1 else ("gather" if self.heads % world else "a2a")
        else:
            self.exchange = mode               # explicit: also honoured by a 1-rank group (exercises the RCCL calls on one GPU)
        self.world = world
        self._load(state_dict, prefix)
        self._rope_cache = {}
        self._time_cache = {}
        self._ctx_cache = {}
        self._ws = {}
        self._mx_act = {}          # mxfp8: (rows, K) -> MxTensor, the quantised A operand of the next block linear
        self.trace = None          # tests: dict filled with per-sub-block activations "block{i}.{j}" -> [S, D]
        # DRN_PER_LAUNCH=1: one ctypes call per kernel (the path the sharded engine and the traces use) instead of the
        # drn_dit_forward sequencer - same kernels, same bits (tests compare the two)
        self._per_launch = os.environ.get("DRN_PER_LAUNCH", "0") == "1"
        # mxfp8: the producers (LayerNorm + modulate, attention, the GELU epilogue of MLP-up) write the quantised operand of the
        # next block linear themselves - no quantise launch, the same bits (drn.h).  DRN_MX_FUSED=0: a quantise launch in front of
        # every block linear (the A/B switch).  Trace mode keeps the bf16 intermediates.
        self._mx_fused = self._mx and os.environ.get("DRN_MX_FUSED", "1") != "0"
        # mxfp8 with the head <-> token exchange: the attention output goes home as e4m3 elements + scales (what its epilogue
        # writes, 0.516 x the bytes of bf16) and the out-projection reads them as they arrive.  DRN_SP_MX_RETURN=0: the bf16 return
        # exchange and a quantise launch (the A/B switch; the same bits)
        self._mx_return = self._mx and os.environ.get("DRN_SP_MX_RETURN", "1") != "0"
        self.sp_path = None        # sharded forwards: which layout / return exchange the last one took (tests, tools)
        # DRN_SP_SPLIT_RETURN=0: the return all-to-all as ONE collective after the whole attention (A/B runs)
        self._split_return = os.environ.get("DRN_SP_SPLIT_RETURN", "1") != "0"
        # step cache (step_cache.py): the controller of the sample loop between cache_begin and cache_end, and the
        # log of the last loop: per step (computed, delta or None)
        self._cache = None
        self.step_cache_log = []

    # ------------------------------------------------------------------ weights
    def _load(self, sd, p):
        dev, bf = self.device, torch.bfloat16

        def g(name):
            return sd[p + name].to(device=dev, dtype=bf)

        self.w_patch = _pad_cols(g("x_embedder.proj.1.weight"), 64)
        self.kpad = self.w_patch.shape[1]
        self.w_t1 = g("t_embedder.1.linear_1.weight").contiguous().unsqueeze(0)
        self.w_t2 = g("t_embedder.1.linear_2.weight").contiguous().unsqueeze(0)
        self.w_affnorm = g("affline_norm.weight").contiguous()
        self.seq = sd[p + "pos_embedder.seq"]
        self.ctx_table = g("context_embedding.weight") if self.use_ctx else None
        self.w_final = _pad_rows(g("final_layer.linear.weight"), 128)
        self.final_cols = self.out_ch * self.ps * self.ps * self.pt
        self.w_fa1 = g("final_layer.adaLN_modulation.1.weight").contiguous().unsqueeze(0)
        self.w_fa2 = g("final_layer.adaLN_modulation.2.weight").contiguous().unsqueeze(0)

        a1, a2 = [], []
        self.blocks = []
        ca_v, ca_o = [], []
        for i in range(self.L):
            subs = []
            for j, kind in enumerate(self.kinds):
                q = f"blocks.block{i}.blocks.{j}."
                a1.append(g(q + "adaLN_modulation.1.weight"))
                a2.append(g(q + "adaLN_modulation.2.weight"))
                if kind == "fa":
                    a = q + "block.attn."
                    wq, wk, wv = g(a + "to_q.0.weight"), g(a + "to_k.0.weight"), g(a + "to_v.0.weight")
                    if self.exchange == "a2a":
                        # K|V output columns grouped by the rank that will own the heads: [rank][k | v][heads/world * 128];
                        # q rows are rank-major as they are (a rank's heads are contiguous).  Kept as [q ; k|v] row blocks.
                        W = self.D // self.world
                        wkv = torch.stack([wk.view(self.world, W, -1), wv.view(self.world, W, -1)], 1).reshape(2 * self.D, -1)
                        wqkv = torch.cat([wq, wkv], 0).contiguous()
                    else:
                        wqkv = torch.cat([wq, wk, wv], 0).contiguous()
                    subs.append({"kind": "fa", "wqkv": wqkv,
                                 "qn": g(a + "to_q.1.weight").contiguous(), "kn": g(a + "to_k.1.weight").contiguous(),
                                 "wo": g(a + "to_out.0.weight").contiguous()})
                elif kind == "ca":
                    a = q + "block.attn."
                    subs.append({"kind": "ca", "idx": len(ca_v)})
                    ca_v.append(g(a + "to_v.0.weight"))
                    ca_o.append(g(a + "to_out.0.weight"))
                else:
                    subs.append({"kind": "mlp", "w1": g(q + "block.layer1.weight").contiguous(),
                                 "w2": g(q + "block.layer2.weight").contiguous()})
            self.blocks.append(subs)
        self.n_sites = len(a1)
        self.r = a1[0].shape[0]
        self.w_a1 = torch.cat(a1, 0).contiguous().unsqueeze(0)          # [1, sites*r, D]
        self.w_a2 = torch.stack(a2, 0).contiguous()                     # [sites, 3D, r]
        self.n_ca = len(ca_v)
        self.w_cav = torch.stack(ca_v, 0).contiguous() if ca_v else None   # [n_ca, D, ctx]
        self.w_cao = torch.stack(ca_o, 0).contiguous() if ca_o else None   # [n_ca, D, D]
        # site index of every cross-attention sub-block (for its gate)
        self.ca_sites = [i * len(self.kinds) + j for i in range(self.L) for j, k in enumerate(self.kinds) if k == "ca"]
        if self._mx:
            # quantise the four block linears once, on the device, and drop their bf16 copies
            for subs in self.blocks:
                for sb in subs:
                    for key in ("wqkv", "wo", "w1", "w2"):
                        if key in sb:
                            sb[key] = N.mx_quant(sb[key])
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
        # the same sub-block list as the host table drn_dit_forward walks (weights never move after load; mxfp8: the e4m3
        # elements and their scale arrays)
        flat = [sb for subs in self.blocks for sb in subs]
        self._subs_c = (N.DitSub * len(flat))()
        for site, sb in enumerate(flat):
            e = self._subs_c[site]
            e.site, e.ca_index = site, -1
            if sb["kind"] == "fa":
                e.kind, e.qn, e.kn = N.SUB_FA, sb["qn"].data_ptr(), sb["kn"].data_ptr()
                wa, wb = sb["wqkv"], sb["wo"]
            elif sb["kind"] == "ca":
                e.kind, e.ca_index = N.SUB_CA, sb["idx"]
            else:
                e.kind = N.SUB_MLP
                wa, wb = sb["w1"], sb["w2"]
            if sb["kind"] != "ca":
                if self._mx:
                    e.w_a, e.w_b, e.s_a, e.s_b = wa.q.data_ptr(), wb.q.data_ptr(), wa.scales.data_ptr(), wb.scales.data_ptr()
                else:
                    e.w_a, e.w_b = wa.data_ptr(), wb.data_ptr()

    # ------------------------------------------------------------------ per-timestep vectors (K10, K11)
    def prepare_timesteps(self, sigmas) -> None:
        """AdaLN vectors of a whole sigma schedule in ONE batched pass (host table -> one H2D copy -> batched GEMVs).

        The sampler knows every sigma before its loop starts; computing their vectors up front keeps host->device copies
        (which block the host until the stream drains) out of the denoising loop, so kernel launches run ahead of the GPU.
        Same arithmetic per sigma as the reference evaluates inside every forward (CleanGeneralDIT.py:664-666, :500-505)."""
        todo = []
        for s_ in sigmas:
            k = float(s_)
            if k not in self._time_cache and k not in todo:
                todo.append(k)
        if not todo:
            return
        D, B = self.D, len(todo)
        t_emb = torch.cat([timestep_sinusoid(k, D) for k in todo], 0).to(self.device)        # [B, D]
        x = t_emb.view(1, B, D)
        h1 = N.gemv(x, self.w_t1)                                                # linear_1
        lora = N.gemv(h1, self.w_t2, act=N.ACT_SILU)                             # linear_2(silu(.))   [1,B,3D]
        emb = N.rmsnorm(t_emb, self.w_affnorm).view(1, B, D)                     # affline_norm
        a = N.gemv(emb, self.w_a1, act=N.ACT_SILU)                               # [1,B,sites*r]
        a = a.view(B, self.n_sites, self.r).permute(1, 0, 2).contiguous()        # [sites,B,r]
        mod = N.gemv(a, self.w_a2, add=lora)                                     # [sites,B,3D]
        af = N.gemv(emb, self.w_fa1, act=N.ACT_SILU)
        modf = N.gemv(af, self.w_fa2, add=lora[:, :, : 2 * D].contiguous())      # [1,B,2D]
        if len(self._time_cache) + B > 512:
            self._time_cache.clear()
        for i, k in enumerate(todo):
            self._time_cache[k] = (mod[:, i, :], modf[0, i])                     # rows stay contiguous: [sites][3D], [2D]

    def time_vectors(self, sigma: float):
        """AdaLN vectors for one sigma: mod [sites, 3D] (shift|scale|gate), final [2D].  Cached per sigma."""
        key = float(sigma)
        hit = self._time_cache.get(key)
        if hit is None:
            self.prepare_timesteps([key])
            hit = self._time_cache[key]
        return hit

    def context_vectors(self, context_index) -> Optional[torch.Tensor]:
        """c_i = to_out_i(to_v_i(ctx)) for every cross-attention block: [n_ca, D].  Cached per index (F8)."""
        if self.n_ca == 0:
            return None
        key = int(context_index) if self.use_ctx else -1
        hit = self._ctx_cache.get(key)
        if hit is not None:
            return hit
        if self.use_ctx:
            ctx = self.ctx_table[key].view(1, 1, self.ctx_dim).contiguous()
        else:
            ctx = torch.zeros((1, 1, self.ctx_dim), dtype=torch.bfloat16, device=self.device)
        v = N.gemv(ctx, self.w_cav)                         # [n_ca,1,D]  to_v (value norm is Identity)
        c = N.gemv(v, self.w_cao).view(self.n_ca, self.D)   # to_out
        self._ctx_cache[key] = c
        return c

    def rope(self, Tp, Hp, Wp):
        key = (Tp, Hp, Wp)
        hit = self._rope_cache.get(key)
        if hit is None:
            cos, sin = rope_cos_sin(Tp, Hp, Wp, 128, self.seq, torch.bfloat16)
            hit = (cos.to(self.device), sin.to(self.device))
            self._rope_cache[key] = hit
        return hit

    def _workspace(self, S, rows, B=1):
        """Activation buffers for `rows` local tokens of S total, B clips stacked along the rows (one shape kept resident): the
        residual stream and the token-local scratch that every exchange needs, then what the configured one adds."""
        key = (S, rows, B)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        D, dev, bf, u8 = self.D, self.device, torch.bfloat16, torch.uint8
        n, hid = B * rows, int(D * self.net["mlp_ratio"])
        ws = {"x": torch.empty((n, D), dtype=bf, device=dev), "h": torch.empty((n, D), dtype=bf, device=dev),
              "o": torch.empty((n, D), dtype=bf, device=dev), "u": torch.empty((n, hid), dtype=bf, device=dev),
              "y": torch.empty((B * S, self.w_final.shape[0]), dtype=bf, device=dev)}
        lib = N.load_library()

        def mx_view(buf, K, q_bytes):
            """[n, K] MXFP8 over a byte buffer laid out as drn_dit_forward takes it: elements from the start, scales from q_bytes."""
            return N.MxTensor(buf[:n * K].view(torch.float8_e4m3fn).view(n, K), buf[q_bytes:q_bytes + n * (K // 32)].view(n, K // 32))
        if self._mx:
            # AQ | AS: the quantised A operand of the next block linear (H or O as MXFP8; sized for the K = hidden operand too)
            ws["act"] = torch.empty(lib.drn_dit_forward_mx_act_bytes(B, rows, D, hid), dtype=u8, device=dev)
            ws["act_mx"] = mx_view(ws["act"], D, n * max(D, hid))
            if self._mx_fused:
                # UQ | US: U as MXFP8 (MLP-up writes it while it reads AQ | AS)
                ws["uact"] = torch.empty(lib.drn_dit_forward_mx_u_bytes(B, rows, hid), dtype=u8, device=dev)
                ws["uact_mx"] = mx_view(ws["uact"], hid, n * hid)
        {"none": self._ws_local, "a2a": self._ws_a2a, "gather": self._ws_gather}[self.exchange](ws, S, rows, B)
        self._ws = {key: ws}
        return ws

    def _mx_attn_views(self, ws, B, S, Da):
        """MXFP8 attention operands of Da / 128 heads over S tokens of B clips: QQ | KQ | VT | QS | KS | VS in one buffer, at the
        offsets drn_dit_forward reads them (drn.h); as (q, k: MxTensor [B * S, Da]; vt, vs of mx_quant_vt)."""
        lay = (ctypes.c_int64 * 8)()
        N._check(N.load_library().drn_dit_forward_mx_attn_layout(B, S, Da, lay), "drn_dit_forward_mx_attn_layout")
        buf = torch.empty(lay[6], dtype=torch.uint8, device=self.device)
        n, heads, Sp = B * S, Da // 128, lay[7]
        shapes = ((n, Da), (n, Da), (B, heads, 128, Sp), (n, Da // 32), (n, Da // 32), (B, heads, 128, Sp // 32))
        views = [buf[off:off + math.prod(shape)].view(shape) for off, shape in zip(lay, shapes)]
        qq, kq, vt = (v.view(torch.float8_e4m3fn) for v in views[:3])
        ws["mx_attn"] = buf
        ws["mx_attn_views"] = (N.MxTensor(qq, views[3]), N.MxTensor(kq, views[4]), vt, views[5])

    def _ws_local(self, ws, S, rows, B):
        """No exchange: the buffers of drn_dit_forward (the per-launch path uses the same ones)."""
        D, dev, hid = self.D, self.device, ws["u"].shape[1]
        lib = N.load_library()
        ws["qkv"] = torch.empty((B * S, 3 * D), dtype=torch.bfloat16, device=dev)      # q | k | v, fused projection
        nb = lib.drn_dit_forward_gemm_workspace_bytes(B, S, D, hid, self.w_final.shape[0], self.kpad)
        if self._mx:
            nb = max(nb, lib.drn_dit_forward_mx_gemm_workspace_bytes(B, S, D, hid))    # the slices of the MXFP8 linears share it
        ws["gemm_ws"] = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None      # split-K partials (few tokens)
        if self._amx:
            self._mx_attn_views(ws, B, S, D)
        nb = lib.drn_dit_forward_attn_workspace_bytes(B, self.heads, S)
        ws["attn_ws"] = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None      # split-KV partials

    def _ws_a2a(self, ws, S, rows, B):
        """Head <-> token all-to-all, one clip at a time: band projections, send / receive slabs, the attention of own heads."""
        D, dev, bf, world = self.D, self.device, torch.bfloat16, self.world
        W = D // world                                                     # columns of this rank's heads
        ws["qb"] = torch.empty((rows, D), dtype=bf, device=dev)            # band projections: [rows][rank][W]
        ws["kvb"] = torch.empty((rows, 2 * D), dtype=bf, device=dev)       #                   [rows][rank][k | v][W]
        ws["sq"] = torch.empty((world, rows, W), dtype=bf, device=dev)     # send slabs, rank-major
        ws["skv"] = torch.empty((world, rows, 2 * W), dtype=bf, device=dev)
        ws["rq"] = torch.empty((S, W), dtype=bf, device=dev)               # all tokens, own heads
        ws["rkv"] = torch.empty((S, 2 * W), dtype=bf, device=dev)
        ws["oh"] = torch.empty((S, W), dtype=bf, device=dev)               # attention output, own heads
        ws["oback"] = torch.empty((world, rows, W), dtype=bf, device=dev)
        if self._mx:
            # the same two as MXFP8 (e4m3 return exchange), and the token-major regroup of the unfused layout
            ws["ohm"] = N.mx_empty(S, W, dev)
            ws["obm"] = N.MxTensor(torch.empty((world, rows, W), dtype=torch.float8_e4m3fn, device=dev),
                                   torch.empty((world, rows, W // 32), dtype=torch.uint8, device=dev))
            ws["otm"] = N.mx_empty(rows, D, dev)
        if self._amx:
            self._mx_attn_views(ws, 1, S, W)                               # Q of all tokens, heads / world heads

    def _ws_gather(self, ws, S, rows, B):
        """K|V all-gather, one clip at a time: local queries against the keys and values of ALL tokens, every head."""
        D, dev, bf = self.D, self.device, torch.bfloat16
        ws["q"] = torch.empty((rows, D), dtype=bf, device=dev)             # local queries
        ws["kv"] = torch.empty((S, 2 * D), dtype=bf, device=dev)           # k | v of ALL tokens (all-gathered)
        if self._amx:
            ws["kb"] = torch.empty((rows, D), dtype=bf, device=dev)        # K of the band (gathered as MXFP8, not as bf16)
            ws["vfull"] = torch.empty((S, D), dtype=bf, device=dev)        # V of ALL tokens (all-gathered)
            self._mx_attn_views(ws, 1, S, D)                               # Q of the band only

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def __call__(self, x, timesteps, latent_condition, context_index=None, **_):
        return self.forward(x, timesteps, latent_condition, context_index)

    @torch.no_grad()
    def forward(self, x, timesteps, latent_condition, context_index=None):
        """net(x, timesteps, latent_condition, context_index) -> [B, out_ch, F, h, w] (full latent on every rank).

        B > 1 stacks B clips of one shape and one sigma along the token rows (row = b*S + s): the G-buffer passes of one
        clip and the cond / uncond halves of classifier-free guidance are such batches.  Every op is
        row-local except self-attention, which runs per clip (batch stride), so each clip's result is that of its own
        B = 1 forward.  `context_index`: int, list of B ints or a [B, 1] tensor; `latent_condition` [B or 1, ...]."""
        dev, bf = self.device, torch.bfloat16
        x = x.to(device=dev, dtype=bf).contiguous()
        cond = latent_condition.to(device=dev, dtype=bf)
        B, C, F_, h, w = x.shape
        if cond.shape[0] == 1 and B > 1:
            cond = cond.expand(B, *cond.shape[1:])
        cond = cond.contiguous()
        if cond.shape[0] != B or tuple(cond.shape[2:]) != (F_, h, w):
            # the reference fails here too: torch.cat of x and latent_condition (CleanGeneralDIT.py:675)
            raise ValueError(f"latent_condition {tuple(cond.shape)} does not match x {tuple(x.shape)} outside the channel dim")
        if C + cond.shape[1] + (1 if self.with_mask else 0) != self.net["in_channels"] + self.net.get("additional_concat_ch", 16) + (1 if self.with_mask else 0):
            raise ValueError("channel count of x | latent_condition does not match the patch-embed weights")
        if torch.is_tensor(timesteps):
            ts = timesteps.flatten().tolist()
            if any(float(t) != float(ts[0]) for t in ts):
                raise ValueError("all clips of a batch share one sigma (the sampler steps them together)")
            sigma = float(ts[0])
        else:
            sigma = float(timesteps)
        cis = [0] * B
        if self.use_ctx:
            if torch.is_tensor(context_index):
                cis = [int(v) for v in context_index.flatten().tolist()]
            elif isinstance(context_index, (list, tuple)):
                cis = [int(v) for v in context_index]
            else:
                cis = [int(context_index)]
            if len(cis) == 1 and B > 1:
                cis = cis * B
            if len(cis) != B:
                raise ValueError(f"context_index has {len(cis)} entries for a batch of {B}")
        D = self.D
        Tp, Hp, Wp = F_ // self.pt, h // self.ps, w // self.ps
        S = Tp * Hp * Wp
        rank, world = group_info(self.pg) if self.pg is not None else (0, 1)
        plan = ShardPlan(S, rank, world)          # (a sharded batch: every clip is cut into the same token bands, rows = b * band + r)

        mod, modf = self.time_vectors(sigma)
        addvec = None
        if self.n_ca:
            gates = mod[self.ca_sites, 2 * D:]                 # [n_ca, D]
            if B == 1:
                addvec = gates * self.context_vectors(cis[0])  # bf16(gate * c): the whole cross-attention block
            else:
                cv = torch.stack([self.context_vectors(c) for c in cis], 1)       # [n_ca, B, D]
                addvec = (gates.unsqueeze(1) * cv).contiguous()
        return self._run(x, cond, mod, modf, addvec, (Tp, Hp, Wp), plan)

    # ------------------------------------------------------------------ step cache
    def _cache_refusals(self):
        if self.trace is not None or self._per_launch:
            raise ValueError("the step cache cuts the one-call forward (drn_dit_forward_range): not with a trace or DRN_PER_LAUNCH=1")

    def cache_begin(self, thr: float, max_run: int, n_steps: int) -> None:
        """Open a sample loop of `n_steps` forwards under the step cache (step_cache.Controller): until cache_end every forward is
        one step of it - the head (patch embed + block 0) always runs, the other blocks only where the probe behind block 0 moved
        by `thr` or more since the last computed step, or the rule forces them.  Two [B S, D] bf16 buffers live from the loop's first
        forward to cache_end; a candidate step reads B x 2 doubles back (its one synchronisation).  A net of fewer than 2 blocks
        ignores the setting."""
        if self.pg is not None:
            raise NotImplementedError("the step cache under sequence parallelism is not implemented: set step_cache = 0")
        self._cache_refusals()
        if self._cache is not None:
            raise RuntimeError("cache_begin inside an open sample loop: call cache_end first")
        self.step_cache_log = []
        if self.L < 2:
            SC.check_step_cache(thr, max_run)
            return
        n_head, n_sub = len(self.kinds), len(self._subs_c)
        cur = {}                                  # what the step in hand works on: args (the sequencer's block), x [B S, D], B

        def part(lo, hi, flags):
            N.dit_forward_range(cur["args"], lo, hi, flags)
            return cur["x"]

        self._cache = SC.Controller(thr, max_run, n_steps, head=lambda _: part(0, n_head, N.DIT_EMBED),
                                    tail=lambda x: part(n_head, n_sub, 0), final=lambda x: part(n_sub, n_sub, N.DIT_FINAL),
                                    backend=_HipCacheBackend(cur))
        self._cache.cur, self._cache.shape = cur, None
        self.step_cache_log = self._cache.log

    def cache_end(self) -> None:
        """Close the sample loop: the two buffers are freed, the log stays in `step_cache_log`."""
        c, self._cache = self._cache, None
        if c is not None:
            c.cur.clear()
            c.end()

    def _lin(self, a, w, out, epilogue=N.EPI_NONE, gate=None, residual=None, rows_per_batch=None):
        """A block linear (q|k|v, out-proj, MLP-up, MLP-down): the bf16 GEMM, or with precision 'mxfp8' the quantisation of
        `a` followed by the MXFP8 GEMM against the weights quantised at load (native.gemm_mxfp8 picks the few-token kernel and its
        K slices from one clip's rows, as drn_dit_forward does)."""
        if not self._mx:
            return N.gemm(a, w, out=out, epilogue=epilogue, gate=gate, residual=residual, rows_per_batch=rows_per_batch)
        return N.gemm_mxfp8(self._mxq(a), w, out=out, epilogue=epilogue, gate=gate, residual=residual,
                            rows_per_batch=rows_per_batch, splitk=None)

    def _mxq(self, a):
        """The MXFP8 operand of a block linear: `a` as it is when a fused producer wrote it as MX already, else the quantise launch
        (into a buffer kept per shape)."""
        if isinstance(a, N.MxTensor):
            return a
        key = tuple(a.shape)
        aq = N.mx_quant(a, out=self._mx_act.get(key))
        self._mx_act[key] = aq
        return aq

    @staticmethod
    def _rows(t, lo, hi):
        """Rows lo .. hi of a bf16 matrix or of an MxTensor (elements and scales): weight row blocks, token bands."""
        return N.MxTensor(t.q[lo:hi], t.scales[lo:hi]) if isinstance(t, N.MxTensor) else t[lo:hi]

    def _lin_planes(self, a, w, out, rows, a_planes=False, c_planes=False, **epi):
        """A block linear that writes (c_planes) or reads (a_planes) the rank-major slabs of the head <-> token all-to-all."""
        if self._mx:
            return N.gemm_mxfp8_blocked(a, w, out, rows, a_planes=a_planes, c_planes=c_planes, **epi)
        return N.gemm_blocked(a, w, out, rows, a_planes=a_planes, c_planes=c_planes, **epi)

    @staticmethod
    def _traced(X, pending, B):
        if pending is None:
            return X.clone()
        return (X.view(B, -1, X.shape[1]) + pending.view(B, 1, -1)).view_as(X)

    @staticmethod
    def _regroup_bytes(src, dst):
        """[world, rows, C] bytes -> [rows, world, C] bytes with the bf16 regroup kernel over byte pairs."""
        world, rows, C = src.shape
        N.permute_021(src.view(torch.uint8).view(torch.bfloat16),
                      out=dst.view(torch.uint8).view(rows, world * C).view(torch.bfloat16))

    def _attend(self, q, k, v, heads, amx, out, part=None):
        """Enqueue the attention of `heads` heads over all keys for the sharded paths, after norm + RoPE.  bf16: q [Sq, heads*128],
        k / v [S, heads*128] views; amx: q / k MxTensors, v = (vt, vs) of mx_quant_vt.  part: one (q0, q1, kv_splits) of
        native.attention_plan, or None for all Sq queries under the automatic plan.  `out` ([Sq, heads*128], bf16 or an MxTensor
        written by the MX epilogue) receives the rows of the queries."""
        q0, q1, ns = part if part is not None else (0, q.shape[0], None)
        o, om = (None, self._rows(out, q0, q1)) if isinstance(out, N.MxTensor) else (out[q0:q1].unsqueeze(0), None)
        if amx:
            N.attention_mxfp8(self._rows(q, q0, q1), k, v[0], v[1], 1, q1 - q0, k.shape[0], out=o, out_mx=om, kv_splits=ns)
        else:
            N.attention(q[q0:q1].unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), out=o, heads=heads, kv_splits=ns, out_mx=om)

    @staticmethod
    def _norm_rope(which, x, w, rope, heads, out_mx=None, **where):
        """RMSNorm + RoPE of the q or the k rows `x` (which: "q" / "k"): in place, or with `out_mx` written there as MXFP8
        (x keeps its input).  where: tokens_per_batch, pos_offset of the rows."""
        xs, ws_ = ((x, None), (w, None)) if which == "q" else ((None, x), (None, w))
        if out_mx is None:
            N.qk_norm_rope(*xs, *ws_, *rope, heads, **where)
        else:
            N.qk_norm_rope_mx(*xs, *ws_, *rope, heads, **where, **{"out_" + which: out_mx})

    def _to_slabs(self, hin, w, band, slabs, route):
        """A projection of the token band into the rank-major send slabs [world, rows, C] of the head <-> token exchange: written
        there by the blocked GEMM, or as the plain GEMM into `band` [rows, world * C] + a regroup pass."""
        world, rows, C = slabs.shape
        if route.layout == "slabs":
            self._lin_planes(hin, w, slabs, rows, c_planes=True)
        else:
            self._lin(hin, w, band)
            N.permute_021(band.view(rows, world, C), out=slabs)

    def _fa_a2a(self, sb, hin, ws, plan, rope, gate, route, b):
        """Self-attention sub-block of clip b's token band with the head <-> token all-to-all, in launch order (hin: modulated input
        of all clips - bf16, or the MxTensor a fused LayerNorm wrote; the residual stream ws["x"] is updated in place).
        tokens -> heads: project the band into rank-major slabs, all-to-all; norm + RoPE + attention over all S tokens of this
        rank's heads; heads -> tokens: all-to-all back, output projection."""
        D, S, rows, world = self.D, plan.S, plan.rows, plan.world
        W, hpr = D // world, self.heads // world
        hin = self._rows(hin, b * rows, (b + 1) * rows)
        if self._mx:
            hin = self._mxq(hin)                                 # one operand for the K|V and the Q projection
        rq, rkv = ws["rq"], ws["rkv"]
        # K|V go first so their exchange (RCCL's stream, 2/3 of the bytes) overlaps the Q projection
        self._to_slabs(hin, self._rows(sb["wqkv"], D, 3 * D), ws["kvb"], ws["skv"], route)
        work_kv = alltoall_rows_(ws["skv"], rkv.view(world, rows, 2 * W), self.pg, async_op=True)
        self._to_slabs(hin, self._rows(sb["wqkv"], 0, D), ws["qb"], ws["sq"], route)
        work_q = alltoall_rows_(ws["sq"], rq.view(world, rows, W), self.pg, async_op=True)
        # amx: q and k leave norm + RoPE as MXFP8, contiguous [S, W]; v is transposed and quantised along the keys
        qm, km, vt, vs = ws["mx_attn_views"] if route.amx else (None,) * 4
        wait_exchange(work_kv, "a2a k|v")
        k, v = rkv[:, :W], rkv[:, W:]
        self._norm_rope("k", k, sb["kn"], rope, hpr, km, tokens_per_batch=S)
        if route.amx:
            N.mx_quant_vt(v.unsqueeze(0), hpr, out=(vt, vs))
        wait_exchange(work_q, "a2a q")
        self._norm_rope("q", rq, sb["qn"], rope, hpr, qm, tokens_per_batch=S)
        qkv = (qm, km, (vt, vs)) if route.amx else (rq, k, v)
        if route.mx_return:
            out, obm = ws["ohm"], ws["obm"]
            send, recv = (out.q.view(world, rows, W), out.scales.view(world, rows, W // 32)), (obm.q, obm.scales)
        else:
            out = ws["oh"]
            send, recv = out.view(world, rows, W), ws["oback"]
        if route.first_bands:
            # the bands whose queries launch 0 has finished go home while launch 1 runs: only the last bands' slabs (1 of 8 at
            # world 8) travel exposed.  Same launches as the single call: same bits
            self._attend(*qkv, hpr, route.amx, out, route.launches[0])
            work0 = alltoall_bands_(send, recv, 0, route.first_bands, self.pg, async_op=True)
            self._attend(*qkv, hpr, route.amx, out, route.launches[1])
            work1 = alltoall_bands_(send, recv, route.first_bands, world, self.pg, async_op=True)
            wait_exchange(work0, "a2a o (return, under the attention tail)")
            wait_exchange(work1, "a2a o (return)")
        else:
            self._attend(*qkv, hpr, route.amx, out)
            wait_exchange(alltoall_rows_(send, recv, self.pg, async_op=True), "a2a o (return)")
        # out-projection from what came home: slabs as A planes, the bytes as they lie (one rank), byte-pair or bf16 regroup
        X = ws["x"][b * rows:(b + 1) * rows]
        res = dict(epilogue=N.EPI_GATE_RES, gate=gate, residual=X)
        if route.layout == "slabs":
            a = obm if route.mx_return else recv
            if self._mx and not route.mx_return:                 # bf16 came home: quantise the slabs where they lie
                aq = self._mxq(a.view(world * rows, W))
                a = N.MxTensor(aq.q.view(world, rows, W), aq.scales.view(world, rows, W // 32))
            self._lin_planes(a, sb["wo"], X, rows, a_planes=True, **res)
        elif route.mx_return:
            otm = ws["otm"]
            if world == 1:
                otm = N.MxTensor(obm.q.view(rows, D), obm.scales.view(rows, D // 32))
            else:
                self._regroup_bytes(obm.q, otm.q)
                self._regroup_bytes(obm.scales, otm.scales)
            self._lin(otm, sb["wo"], X, **res)
        else:
            O = ws["o"][b * rows:(b + 1) * rows]
            N.permute_021(recv, out=O.view(rows, world, W))
            self._lin(O, sb["wo"], X, **res)

    def _fa_gather(self, sb, hin, ws, plan, rope, gate, route, b):
        """Self-attention sub-block of clip b's token band with the K|V all-gather, in launch order (hin, ws["x"] as _fa_a2a).
        Local projections; K|V go first, so their exchange (RCCL's own stream) overlaps the Q projection + q-norm; the wait
        orders the attention of the band's queries over ALL keys after it."""
        D, heads, rows = self.D, self.heads, plan.rows
        X, hin = ws["x"][b * rows:(b + 1) * rows], self._rows(hin, b * rows, (b + 1) * rows)
        if self._mx:
            hin = self._mxq(hin)                                 # one operand for the K|V and the Q projection
        wqkv, q, KV = sb["wqkv"], ws["q"], ws["kv"]
        where = dict(tokens_per_batch=rows, pos_offset=plan.start)
        qm, km, vt, vs = ws["mx_attn_views"] if route.amx else (None,) * 4
        if route.amx:
            # K of the band leaves norm + RoPE as MXFP8 and is gathered like that (half the bytes of the bf16 K gather); V is
            # gathered in bf16 and transposed + quantised along ALL keys afterwards
            qm = self._rows(qm, 0, rows)
            kb, vfull = ws["kb"], ws["vfull"]
            self._lin(hin, self._rows(wqkv, D, 2 * D), kb)
            self._lin(hin, self._rows(wqkv, 2 * D, 3 * D), plan.band(vfull))
            self._norm_rope("k", kb, sb["kn"], rope, heads, self._rows(km, plan.start, plan.stop), **where)
            work = [allgather_rows_(t, plan, self.pg, async_op=True) for t in (km.q, km.scales, vfull)]
            work = [w_ for w_ in work if w_ is not None] or None
        else:
            kv_loc = plan.band(KV)
            self._lin(hin, self._rows(wqkv, D, 3 * D), kv_loc)
            self._norm_rope("k", kv_loc[:, :D], sb["kn"], rope, heads, **where)
            work = allgather_rows_(KV, plan, self.pg, async_op=True)     # the one exchange of the block (xGMI)
        self._lin(hin, self._rows(wqkv, 0, D), q)
        self._norm_rope("q", q, sb["qn"], rope, heads, qm, **where)
        wait_exchange(work, "gather k|v")
        if route.amx:
            N.mx_quant_vt(vfull.unsqueeze(0), heads, out=(vt, vs))
        qkv = (qm, km, (vt, vs)) if route.amx else (q, KV[:, :D], KV[:, D:])
        O = self._rows(ws["act_mx"] if route.o_mx else ws["o"], b * rows, (b + 1) * rows)
        self._attend(*qkv, heads, route.amx, O)
        self._lin(O, sb["wo"], X, epilogue=N.EPI_GATE_RES, gate=gate, residual=X)

    def _sequencer_args(self, ws, P, S, B, *, mod, modf, batched, addvec, rope):
        """The argument block of drn_dit_forward for this workspace (raw pointers: the caller keeps every tensor alive).
        mod / modf: the AdaLN tables of one sigma; batched: None for one clip, else their per-clip expansions (modB, modfB, gateB)
        of _run; rope: (cos, sin)."""
        D = self.D
        X, Hb, O, U, Y = ws["x"], ws["h"], ws["o"], ws["u"], ws["y"]
        a = N.DitForwardArgs()
        a.S, a.B, a.D, a.hidden, a.heads = S, B, D, U.shape[1], self.heads
        a.n_sub, a.subs = len(self._subs_c), self._subs_c
        if B == 1:
            a.shift, a.scale, a.gate = mod.data_ptr(), mod.data_ptr() + 2 * D, mod.data_ptr() + 4 * D
            assert mod.stride(1) == 1
            a.shift_site_stride = a.scale_site_stride = a.gate_site_stride = mod.stride(0)    # (rows of a batched sigma table)
            a.final_shift, a.final_scale = modf.data_ptr(), modf.data_ptr() + 2 * D
        else:
            modB, modfB, gateB = batched
            a.shift, a.scale, a.gate = modB.data_ptr(), modB.data_ptr() + 2 * B * D, gateB.data_ptr()
            a.shift_site_stride = a.scale_site_stride = 2 * B * D
            a.gate_site_stride = B * D
            a.final_shift, a.final_scale = modfB.data_ptr(), modfB.data_ptr() + 2 * B * D
        if addvec is not None:
            a.addvec, a.addvec_stride = addvec.data_ptr(), addvec[0].numel()
        a.cos, a.sin = rope[0].data_ptr(), rope[1].data_ptr()
        a.P, a.kpad, a.w_patch = P.data_ptr(), self.kpad, self.w_patch.data_ptr()
        a.w_final, a.n_final = self.w_final.data_ptr(), self.w_final.shape[0]
        a.X, a.H, a.QKV, a.O, a.U, a.Y = (t.data_ptr() for t in (X, Hb, ws["qkv"], O, U, Y))
        gws, aws = ws["gemm_ws"], ws["attn_ws"]
        a.gemm_ws, a.gemm_ws_bytes = (gws.data_ptr(), gws.numel()) if gws is not None else (None, 0)
        a.attn_ws, a.attn_ws_bytes = (aws.data_ptr(), aws.numel()) if aws is not None else (None, 0)
        a.eps = 1e-6
        if self._mx:
            a.precision = 1
            a.AQ, a.AS = ws["act_mx"].q.data_ptr(), ws["act_mx"].scales.data_ptr()
            a.act_bytes = ws["act"].numel()
            if self._mx_fused:
                a.mx_fused = 1
                a.UQ, a.US = ws["uact_mx"].q.data_ptr(), ws["uact_mx"].scales.data_ptr()
                a.u_act_bytes = ws["uact"].numel()
        if self._amx:
            a.attn_precision = 1
            a.mx_attn, a.mx_attn_bytes = ws["mx_attn"].data_ptr(), ws["mx_attn"].numel()
        return a

    def _fa_local(self, sb, hin, ws, rope, gate, S, B, fusedmx):
        """Self-attention sub-block without an exchange, launch by launch (the launches of drn_dit_forward, in its order).
        hin: the modulated input (bf16 H, or the MxTensor a fused LayerNorm wrote)."""
        D = self.D
        X, O, QKV = ws["x"], ws["o"], ws["qkv"]
        self._lin(hin, sb["wqkv"], QKV, rows_per_batch=S)
        q, k, v = QKV[:, :D], QKV[:, D:2 * D], QKV[:, 2 * D:]
        amx = self._amx and N.attention_mxfp8_choice(self.heads, S)      # per site, from ONE clip's tokens
        # fused producers: O leaves the attention as MXFP8; the 32x32x16 body has no MX epilogue and keeps bf16 + the quantise launch
        omx = ws["act_mx"] if fusedmx and (amx or N.attention_mx_available()) else None
        if amx:
            # MXFP8 attention (the launches of drn_dit_forward with attn_precision 1): q and k leave norm + RoPE
            # as MX (trace mode keeps the bf16 q and k as well), v is transposed and quantised along the keys
            qm, km, vt, vs = ws["mx_attn_views"]
            N.qk_norm_rope_mx(q, k, sb["qn"], sb["kn"], *rope, self.heads, tokens_per_batch=S,
                              write_bf16=self.trace is not None, out_q=qm, out_k=km)
            N.mx_quant_vt(QKV.view(B, S, 3 * D)[:, :, 2 * D:], self.heads, out=(vt, vs))
            oin = N.attention_mxfp8(qm, km, vt, vs, B, S, S, out=None if omx else O.view(B, S, D), out_mx=omx)
        else:
            N.qk_norm_rope(q, k, sb["qn"], sb["kn"], *rope, self.heads, tokens_per_batch=S)
            Q3 = QKV.view(B, S, 3 * D)
            oin = N.attention(Q3[:, :, :D], Q3[:, :, D:2 * D], Q3[:, :, 2 * D:], out=None if omx else O.view(B, S, D),
                              heads=self.heads, out_mx=omx)
        self._lin(oin if omx else O, sb["wo"], X, epilogue=N.EPI_GATE_RES, gate=gate, residual=X, rows_per_batch=S)

    def _mlp(self, sb, hin, ws, gate, rows, fusedmx):
        """GPT-2 feed-forward sub-block.  Fused producers: U leaves MLP-up as MXFP8 where the GELU -> MX epilogue exists; a sliced
        MLP-up keeps bf16 U and the quantise launch inside _lin."""
        X, U = ws["x"], ws["u"]
        uin = U
        if fusedmx and N.mx_gemm_plan(X.shape[0], U.shape[1], self.D, rows) <= 1:
            uin = N.gemm_mxfp8(hin, sb["w1"], epilogue=N.EPI_GELU, rows_per_batch=rows, out_mx=ws["uact_mx"])
        else:
            self._lin(hin, sb["w1"], U, epilogue=N.EPI_GELU, rows_per_batch=rows)
        self._lin(uin, sb["w2"], X, epilogue=N.EPI_GATE_RES, gate=gate, residual=X, rows_per_batch=rows)

    def _run(self, x, cond, mod, modf, addvec, grid, plan):
        """The kernel sequence of one forward (all shapes / pointers fixed for a given input shape).  grid: (Tp, Hp, Wp) patches."""
        D, S, rows, B = self.D, plan.S, plan.rows, x.shape[0]    # (a sharded batch: row = b * band + r)
        if self._cache is not None:
            # a step of a cached sample loop: refused before anything is allocated or launched
            self._cache_refusals()
            if self._cache.shape not in (None, tuple(x.shape)):
                raise ValueError(f"the input shape changed inside a cached sample loop: {self._cache.shape} -> {tuple(x.shape)}")
            self._cache.shape = tuple(x.shape)
        rope = self.rope(*grid)
        ws = self._workspace(S, rows, B)
        X, Hb, Y = ws["x"], ws["h"], ws["y"]
        batched = None
        if B > 1:
            # shift | scale rows per clip for the batched LayerNorm pass: [sites, 2, B, D] (one sigma -> B equal rows), the
            # final layer's [2, B, D], and one gate row per clip: [sites, B, D]
            batched = (mod[:, :2 * D].reshape(-1, 2, 1, D).expand(-1, 2, B, D).contiguous(),
                       modf.view(2, 1, D).expand(2, B, D).contiguous(),
                       mod[:, 2 * D:].reshape(-1, 1, D).expand(-1, B, D).contiguous())
        # mxfp8 with fused producers (the launches of drn_dit_forward with mx_fused): h, O and U leave their producers as MXFP8
        fusedmx = self._mx_fused and self.trace is None
        sharded = self.exchange != "none"
        if sharded:
            # what every self-attention block of this forward does, decided here once; the exchanges (and the projections that
            # write / read their slabs) then run clip by clip on this rank's band of each clip
            route = sp_route(D, self.heads, S, plan.world, self.exchange, self._mx, self._amx, fusedmx, self._mx_return,
                             self._split_return)
            self.sp_path = route.path()
            fa_sharded = self._fa_a2a if self.exchange == "a2a" else self._fa_gather

        # the latent is tiny: every rank patchifies it all and keeps its own token band
        P = N.patchify_concat(x, cond, self.with_mask, self.pt, self.ps, self.kpad)
        if not sharded and self.trace is None and not self._per_launch:
            # one GPU: the whole launch sequence below is enqueued by ONE C call (csrc/dit_forward.hip: same kernels, same
            # arguments, same order -> same bits; ~570 ctypes round trips less per forward)
            args = self._sequencer_args(ws, P, S, B, mod=mod, modf=modf, batched=batched, addvec=addvec, rope=rope)
            if self._cache is None:
                N.dit_forward(args)
            else:
                # one step of the cached loop: the same launches in parts (drn_dit_forward_range), the tail only where it must
                self._cache.cur.update(args=args, x=X, B=B)
                self._cache.step(None)
            return N.unpatchify(Y, B, self.out_ch, *grid, self.pt, self.ps)
        if sharded:
            for b in range(B):                                   # this rank's band of every clip (P holds whole clips)
                N.gemm(plan.band(P[b * S:(b + 1) * S]), self.w_patch, out=X[b * rows:(b + 1) * rows])
        else:
            N.gemm(P, self.w_patch, out=X, rows_per_batch=rows)

        pending = None
        nk = len(self.kinds)
        for site, sb in enumerate(sb for subs in self.blocks for sb in subs):
            m = mod[site]
            shift, scale, gate = m[:D], m[D:2 * D], m[2 * D:]
            if B > 1:
                shift, scale, gate = batched[0][site, 0], batched[0][site, 1], batched[2][site]
            if self.trace is not None and site > 0:
                self.trace[f"block{(site - 1) // nk}.{(site - 1) % nk}"] = self._traced(X, pending, B)
            if sb["kind"] == "ca":
                if pending is not None:
                    N.bcast_add(X, pending, rows_per_batch=rows)
                pending = addvec[sb["idx"]]
                continue
            if fusedmx:
                hin = N.ln_modulate(X, shift, scale, add_vec=pending, rows_per_batch=rows, out_mx=ws["act_mx"])
            else:
                hin = N.ln_modulate(X, shift, scale, out=Hb, add_vec=pending, rows_per_batch=rows)
            pending = None
            if sb["kind"] == "mlp":
                self._mlp(sb, hin, ws, gate, rows, fusedmx)
            elif not sharded:
                self._fa_local(sb, hin, ws, rope, gate, S, B, fusedmx)
            else:
                for b in range(B):                               # every clip of a batch has the same sigma: the same gate row
                    fa_sharded(sb, hin, ws, plan, rope, m[2 * D:], route, b)

        if self.trace is not None:
            site = len(self.blocks) * nk
            self.trace[f"block{(site - 1) // nk}.{(site - 1) % nk}"] = self._traced(X, pending, B)
        self._final_layer(ws, plan, (modf[:D], modf[D:]) if B == 1 else batched[1], pending, B)
        return N.unpatchify(Y, B, self.out_ch, *grid, self.pt, self.ps)

    def _final_layer(self, ws, plan, mod, pending, B):
        """Final LayerNorm (mod: shift, scale - one row, or one per clip) + projection into ws["y"]."""
        S, rows, Hb, Y = plan.S, plan.rows, ws["h"], ws["y"]
        N.ln_modulate(ws["x"], mod[0], mod[1], out=Hb, add_vec=pending, rows_per_batch=rows)
        if self.exchange != "none" or B == 1:
            # this rank's band of every clip, then every rank gets the full latent (2.4 MB at cfg 3).  One clip without an
            # exchange: the same GEMM; its gather is issued by a 1-rank group under parallel.SINGLE_RANK_COLLECTIVES alone
            for b in range(B):
                Yb = Y[b * S:(b + 1) * S]
                N.gemm(Hb[b * rows:(b + 1) * rows], self.w_final, out=plan.band(Yb))
                allgather_rows_(Yb, plan, self.pg)
        else:
            N.gemm(Hb, self.w_final, out=Y, rows_per_batch=rows)
