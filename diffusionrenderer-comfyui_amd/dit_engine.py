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
from typing import Dict, Optional

import torch

from . import native as N
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
        """Activation buffers for `rows` local tokens of S total, B clips stacked along the rows (one shape kept resident)."""
        key = (S, rows, B)
        ws = self._ws.get(key)
        if ws is None:
            D, dev, bf = self.D, self.device, torch.bfloat16
            n = B * rows
            ws = {"x": torch.empty((n, D), dtype=bf, device=dev), "h": torch.empty((n, D), dtype=bf, device=dev),
                  "o": torch.empty((n, D), dtype=bf, device=dev),
                  "u": torch.empty((n, int(D * self.net["mlp_ratio"])), dtype=bf, device=dev),
                  "y": torch.empty((B * S, self.w_final.shape[0]), dtype=bf, device=dev)}
            lib = N.load_library()
            u8, f8 = torch.uint8, torch.float8_e4m3fn
            if self.exchange != "none" and self._mx:
                # sharded mxfp8: AQ | AS and UQ | US for this rank's band rows of every clip, laid out as on one GPU
                hid = ws["u"].shape[1]
                ws["act"] = torch.empty(lib.drn_dit_forward_mx_act_bytes(B, rows, D, hid), dtype=u8, device=dev)
                ws["act_q_bytes"] = n * max(D, hid)
                if self._mx_fused:
                    ws["uact"] = torch.empty(lib.drn_dit_forward_mx_u_bytes(B, rows, hid), dtype=u8, device=dev)
                    ws["uact_q_bytes"] = n * hid
            if self.exchange != "none" and self._amx:
                # MXFP8 attention over all S keys of the heads this rank attends (a2a: heads / world, Q of all tokens; gather: every
                # head, Q of the band only): QQ | KQ | VT | QS | KS | VS by the layout rule of drn_dit_forward, one clip at a time
                Da = D // self.world if self.exchange == "a2a" else D
                lay = (ctypes.c_int64 * 8)()
                N._check(lib.drn_dit_forward_mx_attn_layout(1, S, Da, lay), "drn_dit_forward_mx_attn_layout")
                buf = torch.empty(lay[6], dtype=u8, device=dev)
                Sp = lay[7]
                shapes = ((S, Da), (S, Da), (1, Da // 128, 128, Sp), (S, Da // 32), (S, Da // 32), (1, Da // 128, 128, Sp // 32))
                views = [buf[off:off + math.prod(shape)].view(shape) for off, shape in zip(lay, shapes)]
                ws["mx_attn"] = buf
                ws["mx_attn_views"] = (N.MxTensor(views[0].view(f8), views[3]), N.MxTensor(views[1].view(f8), views[4]),
                                       views[2].view(f8), views[5])
            if self.exchange == "none":
                ws["qkv"] = torch.empty((B * S, 3 * D), dtype=bf, device=dev)      # q | k | v, fused projection
                nb = lib.drn_dit_forward_gemm_workspace_bytes(B, S, D, ws["u"].shape[1], self.w_final.shape[0], self.kpad)
                if self._mx:
                    # the slices of the MXFP8 block linears share gemm_ws; AQ | AS: the quantised A operand of the next one
                    nb = max(nb, lib.drn_dit_forward_mx_gemm_workspace_bytes(B, S, D, ws["u"].shape[1]))
                    kmax = max(D, ws["u"].shape[1])
                    ws["act"] = torch.empty(lib.drn_dit_forward_mx_act_bytes(B, S, D, ws["u"].shape[1]), dtype=torch.uint8, device=dev)
                    ws["act_q_bytes"] = n * kmax
                    if self._mx_fused:
                        # UQ | US: U as MXFP8 (MLP-up writes it while it reads AQ | AS)
                        ws["uact"] = torch.empty(lib.drn_dit_forward_mx_u_bytes(B, S, ws["u"].shape[1]), dtype=torch.uint8, device=dev)
                        ws["uact_q_bytes"] = n * ws["u"].shape[1]
                ws["gemm_ws"] = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None      # split-K partials (few tokens)
                if self._amx:
                    # MXFP8 attention: QQ | KQ | VT | QS | KS | VS in one buffer, at the offsets drn_dit_forward reads them (drn.h)
                    lay = (ctypes.c_int64 * 8)()
                    N._check(lib.drn_dit_forward_mx_attn_layout(B, S, D, lay), "drn_dit_forward_mx_attn_layout")
                    buf = torch.empty(lay[6], dtype=torch.uint8, device=dev)
                    Sp = lay[7]
                    shapes = ((n, D), (n, D), (B, self.heads, 128, Sp), (n, D // 32), (n, D // 32), (B, self.heads, 128, Sp // 32))
                    views = [buf[off:off + math.prod(shape)].view(shape) for off, shape in zip(lay, shapes)]
                    qq, kq, vt = (v.view(torch.float8_e4m3fn) for v in views[:3])
                    ws["mx_attn"] = buf
                    ws["mx_attn_views"] = (N.MxTensor(qq, views[3]), N.MxTensor(kq, views[4]), vt, views[5])
                nb = lib.drn_dit_forward_attn_workspace_bytes(B, self.heads, S)
                ws["attn_ws"] = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None      # split-KV partials
            elif self.exchange == "a2a":
                W = D // self.world                                                # columns of this rank's heads
                ws["qb"] = torch.empty((rows, D), dtype=bf, device=dev)            # band projections: [rows][rank][W]
                ws["kvb"] = torch.empty((rows, 2 * D), dtype=bf, device=dev)       #                   [rows][rank][k | v][W]
                ws["sq"] = torch.empty((self.world, rows, W), dtype=bf, device=dev)        # send slabs, rank-major
                ws["skv"] = torch.empty((self.world, rows, 2 * W), dtype=bf, device=dev)
                ws["rq"] = torch.empty((S, W), dtype=bf, device=dev)               # all tokens, own heads
                ws["rkv"] = torch.empty((S, 2 * W), dtype=bf, device=dev)
                ws["oh"] = torch.empty((S, W), dtype=bf, device=dev)               # attention output, own heads
                ws["oback"] = torch.empty((self.world, rows, W), dtype=bf, device=dev)
                if self._mx:
                    # the same two as MXFP8 (e4m3 return exchange), and the token-major regroup of the unfused layout
                    ws["ohm"] = N.mx_empty(S, W, dev)
                    ws["obm"] = N.MxTensor(torch.empty((self.world, rows, W), dtype=f8, device=dev),
                                           torch.empty((self.world, rows, W // 32), dtype=u8, device=dev))
                    ws["otm"] = N.mx_empty(rows, D, dev)
            else:
                ws["q"] = torch.empty((rows, D), dtype=bf, device=dev)             # local queries
                ws["kv"] = torch.empty((S, 2 * D), dtype=bf, device=dev)           # k | v of ALL tokens (all-gathered)
                if self._amx:
                    ws["kb"] = torch.empty((rows, D), dtype=bf, device=dev)        # K of the band (gathered as MXFP8, not as bf16)
                    ws["vfull"] = torch.empty((S, D), dtype=bf, device=dev)        # V of ALL tokens (all-gathered)
            self._ws = {key: ws}
        return ws

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
        return self._run(x, cond, mod, modf, addvec, Tp, Hp, Wp, plan)

    @staticmethod
    def _mx_view(buf, q_bytes, rows, K):
        """An MxTensor [rows, K] over a byte buffer laid out as drn_dit_forward is given AQ | AS / UQ | US: elements from the
        start, scales from byte `q_bytes` (the offset the sequencer path passes as AS / US)."""
        return N.MxTensor(buf[:rows * K].view(torch.float8_e4m3fn).view(rows, K),
                          buf[q_bytes:q_bytes + rows * (K // 32)].view(rows, K // 32))

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

    def _attend(self, q, k, v, heads, S, amx, launches, out, out_mx):
        """The attention launches of `heads` heads over all S keys for the sharded paths, after norm + RoPE.  bf16: q [Sq, heads*128],
        k / v [S, heads*128] views; amx: q / k MxTensors, v = (vt, vs) of mx_quant_vt.  launches: [(q0, q1, kv_splits)], or None
        for the one call under the automatic plan.  The output goes to `out` (bf16 [Sq, heads*128]) or `out_mx` (an MxTensor).
        A generator: it yields after every launch, so the caller can start the exchange of the rows that are finished."""
        Sq = q.shape[0]
        for q0, q1, ns in (launches if launches is not None else [(0, Sq, None)]):
            o = out[q0:q1].unsqueeze(0) if out is not None else None
            om = self._rows(out_mx, q0, q1) if out_mx is not None else None
            if amx:
                N.attention_mxfp8(self._rows(q, q0, q1), k, v[0], v[1], 1, q1 - q0, S, out=o, out_mx=om, kv_splits=ns)
            else:
                N.attention(q[q0:q1].unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), out=o, heads=heads, kv_splits=ns, out_mx=om)
            yield q1

    def _fa_sharded(self, sb, hin, X, O, ws, plan, cos, sin, gate, fused, omx):
        """Self-attention sub-block of ONE clip's token band with an exchange (hin: modulated input rows - bf16, or the MxTensor a
        fused LayerNorm wrote; X: residual stream rows, updated in place; O: scratch rows; omx: their MXFP8 twin or None)."""
        D = self.D
        S, rows, world = plan.S, plan.rows, plan.world
        mx = self._mx
        if mx:
            hin = self._mxq(hin)                                 # one operand for the K|V and the Q projection
        wq, wkv, wo = self._rows(sb["wqkv"], 0, D), self._rows(sb["wqkv"], D, 3 * D), sb["wo"]
        res = dict(epilogue=N.EPI_GATE_RES, gate=gate, residual=X)
        if self.exchange == "a2a":
            # tokens -> heads: project the band, regroup rank-major, all-to-all; norm + RoPE + attention over all S
            # tokens of this rank's heads; heads -> tokens: all-to-all back, regroup, output projection.
            # K|V go first so their exchange (RCCL's stream, 2/3 of the bytes) overlaps the Q projection.
            W, hpr = D // world, self.heads // world
            Oh, oback, rq, rkv = ws["oh"], ws["oback"], ws["rq"], ws["rkv"]
            amx = self._amx and N.attention_mxfp8_choice(hpr, S)               # per site, from ONE clip's tokens
            # (the projections write the rank-major send slabs themselves where the tile kernel can; else a regroup pass)
            if fused:
                self._lin_planes(hin, wkv, ws["skv"], rows, c_planes=True)
            else:
                self._lin(hin, wkv, ws["kvb"])
                N.permute_021(ws["kvb"].view(rows, world, 2 * W), out=ws["skv"])
            work_kv = alltoall_rows_(ws["skv"], rkv.view(world, rows, 2 * W), self.pg, async_op=True)
            if fused:
                self._lin_planes(hin, wq, ws["sq"], rows, c_planes=True)
            else:
                self._lin(hin, wq, ws["qb"])
                N.permute_021(ws["qb"].view(rows, world, W), out=ws["sq"])
            work_q = alltoall_rows_(ws["sq"], rq.view(world, rows, W), self.pg, async_op=True)
            wait_exchange(work_kv, "a2a k|v")
            k, v = rkv[:, :W], rkv[:, W:]
            if amx:
                # q and k leave norm + RoPE as MXFP8, contiguous [S, W]; v is transposed and quantised along the keys
                qm, km, vt, vs = ws["mx_attn_views"]
                N.qk_norm_rope_mx(None, k, None, sb["kn"], cos, sin, hpr, tokens_per_batch=S, out_k=km)
                N.mx_quant_vt(v.unsqueeze(0), hpr, out=(vt, vs))
                wait_exchange(work_q, "a2a q")
                N.qk_norm_rope_mx(rq, None, sb["qn"], None, cos, sin, hpr, tokens_per_batch=S, out_q=qm)
                aq, ak, av = qm, km, (vt, vs)
            else:
                N.qk_norm_rope(None, k, None, sb["kn"], cos, sin, hpr, tokens_per_batch=S)
                wait_exchange(work_q, "a2a q")
                N.qk_norm_rope(rq, None, sb["qn"], None, cos, sin, hpr, tokens_per_batch=S)
                aq, ak, av = rq, k, v
            # mxfp8: the output leaves the attention as e4m3 + scales and travels like that, where an MX epilogue exists and the
            # receive side can consume the bytes as they are: as A planes (fused), as they lie (one rank), or through the regroup
            # kernel over byte pairs (scale rows of a multiple of 16 bytes); else bf16 goes home and is quantised there
            mxret = (self._mx_return and (amx or N.attention_mx_available())
                     and (fused or world == 1 or (W // 32) % 16 == 0))
            self.sp_path = {"layout": "slabs" if fused else "regroup", "return": "e4m3" if mxret else "bf16",
                            "attention": "mxfp8" if amx else "bf16"}
            if mxret:
                ohm, obm = ws["ohm"], ws["obm"]
                send = (ohm.q.view(world, rows, W), ohm.scales.view(world, rows, W // 32))
                recv = (obm.q, obm.scales)
            else:
                send, recv = Oh.view(world, rows, W), oback
            # heads -> tokens.  The attention of a rank's heads is usually two launches (native.attention_plan: the
            # q-blocks that fill whole rounds of the CUs, then the rest with its keys split): the token bands whose
            # queries the first launch has finished go home while the second one runs, only the last bands' slabs
            # (1 of 8 at world 8) travel exposed.  Same launches as the single call: same bits.
            aplan = N.attention_plan(1, hpr, S, S)
            nb = aplan[0][1] // rows if len(aplan) == 2 else 0             # complete bands of the first launch
            split = nb >= 1 and self._split_return
            att = self._attend(aq, ak, av, hpr, S, amx, aplan if split else None, None if mxret else Oh,
                               ws["ohm"] if mxret else None)
            if split:
                next(att)
                work0 = alltoall_bands_(send, recv, 0, nb, self.pg, async_op=True)
                next(att)
                work1 = alltoall_bands_(send, recv, nb, world, self.pg, async_op=True)
                wait_exchange(work0, "a2a o (return, under the attention tail)")
                wait_exchange(work1, "a2a o (return)")
            else:
                next(att)
                work = alltoall_rows_(send, recv, self.pg, async_op=True)
                wait_exchange(work, "a2a o (return)")
            att.close()
            if fused:
                if mxret:
                    a = ws["obm"]
                elif mx:                                         # bf16 came home: quantise the slabs where they lie
                    aq = self._mxq(oback.view(world * rows, W))
                    a = N.MxTensor(aq.q.view(world, rows, W), aq.scales.view(world, rows, W // 32))
                else:
                    a = oback
                self._lin_planes(a, wo, X, rows, a_planes=True, **res)
                return
            if mxret:
                otm = ws["otm"]
                if world == 1:
                    otm = N.MxTensor(ws["obm"].q.view(rows, D), ws["obm"].scales.view(rows, D // 32))
                else:
                    self._regroup_bytes(ws["obm"].q, otm.q)
                    self._regroup_bytes(ws["obm"].scales, otm.scales)
                self._lin(otm, wo, X, **res)
                return
            N.permute_021(oback, out=O.view(rows, world, W))
        else:
            # local projections; K|V land directly in this rank's band of the gather buffer.  K|V first, so the
            # exchange (RCCL's own stream) overlaps the Q projection + q-norm; wait() orders attention after it.
            q, KV = ws["q"], ws["kv"]
            amx = self._amx and N.attention_mxfp8_choice(self.heads, S)
            self.sp_path = {"layout": "gather", "return": "none", "attention": "mxfp8" if amx else "bf16"}
            if amx:
                # K of the band leaves norm + RoPE as MXFP8 and is gathered like that (half the bytes of the bf16 K gather); V is
                # gathered in bf16 and transposed + quantised along ALL keys afterwards
                qm, km, vt, vs = ws["mx_attn_views"]
                qm = self._rows(qm, 0, rows)
                kb, vfull = ws["kb"], ws["vfull"]
                self._lin(hin, self._rows(sb["wqkv"], D, 2 * D), kb)
                self._lin(hin, self._rows(sb["wqkv"], 2 * D, 3 * D), plan.band(vfull))
                N.qk_norm_rope_mx(None, kb, None, sb["kn"], cos, sin, self.heads, tokens_per_batch=rows, pos_offset=plan.start,
                                  out_k=self._rows(km, plan.start, plan.stop))
                work = [allgather_rows_(t, plan, self.pg, async_op=True) for t in (km.q, km.scales, vfull)]
                work = [w_ for w_ in work if w_ is not None] or None
            else:
                kv_loc = plan.band(KV)
                self._lin(hin, wkv, kv_loc)
                N.qk_norm_rope(None, kv_loc[:, :D], None, sb["kn"], cos, sin, self.heads,
                               tokens_per_batch=rows, pos_offset=plan.start)
                work = allgather_rows_(KV, plan, self.pg, async_op=True)     # the one exchange of the block (xGMI)
            self._lin(hin, wq, q)
            if amx:
                N.qk_norm_rope_mx(q, None, sb["qn"], None, cos, sin, self.heads, tokens_per_batch=rows, pos_offset=plan.start,
                                  out_q=qm)
                wait_exchange(work, "gather k|v")
                N.mx_quant_vt(vfull.unsqueeze(0), self.heads, out=(vt, vs))
                aq, ak, av = qm, km, (vt, vs)
            else:
                N.qk_norm_rope(q, None, sb["qn"], None, cos, sin, self.heads, tokens_per_batch=rows, pos_offset=plan.start)
                wait_exchange(work, "gather k|v")
                aq, ak, av = q, KV[:, :D], KV[:, D:]
            # fused producers: O leaves the attention as MXFP8 (the 32x32x16 body has no MX epilogue: bf16 + the quantise launch)
            if omx is not None and not (amx or N.attention_mx_available()):
                omx = None
            for _ in self._attend(aq, ak, av, self.heads, S, amx, None, None if omx is not None else O, omx):
                pass
            if omx is not None:
                O = omx
        self._lin(O, wo, X, **res)

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
            a.AQ, a.AS = ws["act"].data_ptr(), ws["act"].data_ptr() + ws["act_q_bytes"]
            a.act_bytes = ws["act"].numel()
            if self._mx_fused:
                a.mx_fused = 1
                a.UQ, a.US = ws["uact"].data_ptr(), ws["uact"].data_ptr() + ws["uact_q_bytes"]
                a.u_act_bytes = ws["uact"].numel()
        if self._amx:
            a.attn_precision = 1
            a.mx_attn, a.mx_attn_bytes = ws["mx_attn"].data_ptr(), ws["mx_attn"].numel()
        return a

    def _fa_local(self, sb, hin, ws, cos, sin, gate, S, B, fusedmx):
        """Self-attention sub-block without an exchange, launch by launch (the launches of drn_dit_forward, in its order).
        hin: the modulated input (bf16 H, or the MxTensor a fused LayerNorm wrote)."""
        D = self.D
        X, O, QKV = ws["x"], ws["o"], ws["qkv"]
        self._lin(hin, sb["wqkv"], QKV, rows_per_batch=S)
        q, k, v = QKV[:, :D], QKV[:, D:2 * D], QKV[:, 2 * D:]
        amx = self._amx and N.attention_mxfp8_choice(self.heads, S)      # per site, from ONE clip's tokens
        # fused producers: O leaves the attention as MXFP8; the 32x32x16 body has no MX epilogue and keeps bf16 + the quantise launch
        omx = (self._mx_view(ws["act"], ws["act_q_bytes"], X.shape[0], D)
               if fusedmx and (amx or N.attention_mx_available()) else None)
        if amx:
            # MXFP8 attention (the launches of drn_dit_forward with attn_precision 1): q and k leave norm + RoPE
            # as MX (trace mode keeps the bf16 q and k as well), v is transposed and quantised along the keys
            qm, km, vt, vs = ws["mx_attn_views"]
            N.qk_norm_rope_mx(q, k, sb["qn"], sb["kn"], cos, sin, self.heads, tokens_per_batch=S,
                              write_bf16=self.trace is not None, out_q=qm, out_k=km)
            N.mx_quant_vt(QKV.view(B, S, 3 * D)[:, :, 2 * D:], self.heads, out=(vt, vs))
            oin = N.attention_mxfp8(qm, km, vt, vs, B, S, S, out=None if omx else O.view(B, S, D), out_mx=omx)
        else:
            N.qk_norm_rope(q, k, sb["qn"], sb["kn"], cos, sin, self.heads, tokens_per_batch=S)
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
            uin = N.gemm_mxfp8(hin, sb["w1"], epilogue=N.EPI_GELU, rows_per_batch=rows,
                               out_mx=self._mx_view(ws["uact"], ws["uact_q_bytes"], X.shape[0], U.shape[1]))
        else:
            self._lin(hin, sb["w1"], U, epilogue=N.EPI_GELU, rows_per_batch=rows)
        self._lin(uin, sb["w2"], X, epilogue=N.EPI_GATE_RES, gate=gate, residual=X, rows_per_batch=rows)

    def _run(self, x, cond, mod, modf, addvec, Tp, Hp, Wp, plan):
        """The kernel sequence of one forward (all shapes / pointers fixed for a given input shape)."""
        D = self.D
        S, rows, world = plan.S, plan.rows, plan.world
        B = x.shape[0]                                           # B > 1 only without an exchange (rows == S)
        cos, sin = self.rope(Tp, Hp, Wp)
        ws = self._workspace(S, rows, B)
        X, Hb, O, Y = ws["x"], ws["h"], ws["o"], ws["y"]
        modB = modfB = gateB = None
        if B > 1:
            # shift | scale rows per clip for the batched LayerNorm pass: [sites, 2, B, D] (one sigma -> B equal rows)
            modB = mod[:, :2 * D].reshape(-1, 2, 1, D).expand(-1, 2, B, D).contiguous()
            modfB = modf.view(2, 1, D).expand(2, B, D).contiguous()
            gateB = mod[:, 2 * D:].reshape(-1, 1, D).expand(-1, B, D).contiguous()     # one gate row per clip: [sites, B, D]

        # the latent is tiny: every rank patchifies it all and keeps its own token band
        P = N.patchify_concat(x, cond, self.with_mask, self.pt, self.ps, self.kpad)
        sharded = self.exchange != "none"
        if not sharded and self.trace is None and not self._per_launch:
            # one GPU: the whole launch sequence below is enqueued by ONE C call (csrc/dit_forward.hip: same kernels, same
            # arguments, same order -> same bits; ~570 ctypes round trips less per forward)
            N.dit_forward(self._sequencer_args(ws, P, S, B, mod=mod, modf=modf, batched=(modB, modfB, gateB) if B > 1 else None,
                                               addvec=addvec, rope=(cos, sin)))
            return N.unpatchify(Y, B, self.out_ch, Tp, Hp, Wp, self.pt, self.ps)
        if sharded and B > 1:
            for b in range(B):                                   # this rank's band of every clip (P holds whole clips)
                N.gemm(plan.band(P[b * S:(b + 1) * S]), self.w_patch, out=X[b * rows:(b + 1) * rows])
        else:
            N.gemm(plan.band(P) if B == 1 else P, self.w_patch, out=X, rows_per_batch=rows)

        pending = None
        nk = len(self.kinds)
        fused = None                                             # a2a exchange: blocked-layout GEMMs instead of regroup passes
        # mxfp8 with fused producers (the launches of drn_dit_forward with mx_fused, in its order): h, O and U leave their
        # producers as MXFP8
        fusedmx = self._mx_fused and self.trace is None
        for site, sb in enumerate(sb for subs in self.blocks for sb in subs):
            m = mod[site]
            shift, scale, gate = m[:D], m[D:2 * D], m[2 * D:]
            if B > 1:
                shift, scale, gate = modB[site, 0], modB[site, 1], gateB[site]
            if self.trace is not None and site > 0:
                self.trace[f"block{(site - 1) // nk}.{(site - 1) % nk}"] = self._traced(X, pending, B)
            if sb["kind"] == "ca":
                if pending is not None:
                    N.bcast_add(X, pending, rows_per_batch=rows)
                pending = addvec[sb["idx"]]
                continue
            if fusedmx:
                hin = N.ln_modulate(X, shift, scale, add_vec=pending, rows_per_batch=rows,
                                    out_mx=self._mx_view(ws["act"], ws["act_q_bytes"], X.shape[0], D))
            else:
                hin = N.ln_modulate(X, shift, scale, out=Hb, add_vec=pending, rows_per_batch=rows)
            pending = None
            if sb["kind"] == "mlp":
                self._mlp(sb, hin, ws, gate, rows, fusedmx)
            elif not sharded:
                self._fa_local(sb, hin, ws, cos, sin, gate, S, B, fusedmx)
            else:
                # sharded: the exchanges (and the projections that write / read their slabs) run clip by clip on this
                # rank's band of each clip; every clip of a batch has the same sigma, hence the same gate row
                if fused is None:
                    W_ = D // world
                    if self._mx:
                        # the MXFP8 slab GEMM always runs on the 256 x 256 kernel: taken where the plan of one clip's band rows picks
                        # that kernel anyway (the slab layout then changes no bit) and the planes meet its contract (drn.h)
                        fused = (self.exchange == "a2a" and world > 1 and W_ >= 256 and W_ & (W_ - 1) == 0
                                 and N.mx_gemm_plan(rows, 2 * D, D) == 0 and N.mx_gemm_plan(rows, D, D) == 0)
                    else:
                        fused = (self.exchange == "a2a" and world > 1 and W_ >= 512 and N.gemm_blocked_ok(rows, 2 * D)
                                 and N.gemm_blocked_ok(rows, D))
                omx = self._mx_view(ws["act"], ws["act_q_bytes"], X.shape[0], D) if fusedmx and self.exchange == "gather" else None
                for b in range(B):
                    self._fa_sharded(sb, self._rows(hin, b * rows, (b + 1) * rows), X[b * rows:(b + 1) * rows],
                                     O[b * rows:(b + 1) * rows], ws, plan, cos, sin, m[2 * D:], fused,
                                     self._rows(omx, b * rows, (b + 1) * rows) if omx is not None else None)

        if self.trace is not None:
            site = len(self.blocks) * nk
            self.trace[f"block{(site - 1) // nk}.{(site - 1) % nk}"] = self._traced(X, pending, B)
        if B == 1:
            N.ln_modulate(X, modf[:D], modf[D:], out=Hb, add_vec=pending)
            N.gemm(Hb, self.w_final, out=plan.band(Y))
            allgather_rows_(Y, plan, self.pg)                       # 2.4 MB at cfg 3: every rank gets the full latent
        elif sharded:
            N.ln_modulate(X, modfB[0], modfB[1], out=Hb, add_vec=pending, rows_per_batch=rows)
            for b in range(B):
                Yb = Y[b * S:(b + 1) * S]
                N.gemm(Hb[b * rows:(b + 1) * rows], self.w_final, out=plan.band(Yb))
                allgather_rows_(Yb, plan, self.pg)
        else:
            N.ln_modulate(X, modfB[0], modfB[1], out=Hb, add_vec=pending, rows_per_batch=rows)
            N.gemm(Hb, self.w_final, out=Y, rows_per_batch=rows)
        return N.unpatchify(Y, B, self.out_ch, Tp, Hp, Wp, self.pt, self.ps)
