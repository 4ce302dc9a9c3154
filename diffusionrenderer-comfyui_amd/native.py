"""ctypes binding of libdrn.so (the C ABI of include/drn.h).

PyTorch-ROCm tensors in, raw device pointers + shapes + the current HIP stream out.
There is NO fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

import torch

_LIB = None
_LIB_NAME = "libdrn.so"

EPI_NONE, EPI_GELU, EPI_GATE_RES = 0, 1, 2
ACT_NONE, ACT_SILU = 0, 1

_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float

SUB_FA, SUB_CA, SUB_MLP = 0, 1, 2


class DitSub(Structure):                      # drn_dit_sub (include/drn.h)
    _fields_ = [("kind", c_int32), ("site", c_int32), ("ca_index", c_int32), ("reserved", c_int32),
                ("w_a", c_void_p), ("w_b", c_void_p), ("qn", c_void_p), ("kn", c_void_p),
                ("s_a", c_void_p), ("s_b", c_void_p)]


class DitForwardArgs(Structure):              # drn_dit_forward_args (include/drn.h), field for field
    _fields_ = [("struct_bytes", c_int64), ("S", c_int64), ("B", c_int64), ("D", c_int64), ("hidden", c_int64),
                ("heads", c_int32), ("n_sub", c_int32), ("subs", POINTER(DitSub)),
                ("shift", c_void_p), ("scale", c_void_p), ("gate", c_void_p),
                ("shift_site_stride", c_int64), ("scale_site_stride", c_int64), ("gate_site_stride", c_int64),
                ("addvec", c_void_p), ("addvec_stride", c_int64), ("cos", c_void_p), ("sin", c_void_p),
                ("P", c_void_p), ("kpad", c_int64), ("w_patch", c_void_p),
                ("final_shift", c_void_p), ("final_scale", c_void_p), ("w_final", c_void_p), ("n_final", c_int64),
                ("X", c_void_p), ("H", c_void_p), ("QKV", c_void_p), ("O", c_void_p), ("U", c_void_p), ("Y", c_void_p),
                ("gemm_ws", c_void_p), ("gemm_ws_bytes", c_int64), ("attn_ws", c_void_p), ("attn_ws_bytes", c_int64),
                ("timer", c_void_p), ("eps", c_float), ("precision", c_int32),
                ("AQ", c_void_p), ("AS", c_void_p), ("act_bytes", c_int64),
                ("mx_fused", c_int32), ("reserved", c_int32), ("UQ", c_void_p), ("US", c_void_p), ("u_act_bytes", c_int64),
                ("attn_precision", c_int32), ("reserved2", c_int32), ("mx_attn", c_void_p), ("mx_attn_bytes", c_int64)]


class GbufferEditMap(Structure):              # drn_gbuffer_edit_map (include/drn.h), field for field
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("layer", c_void_p),
                ("src_bs", c_int64), ("src_ts", c_int64), ("dst_bs", c_int64), ("dst_ts", c_int64),
                ("layer_bs", c_int64), ("layer_ts", c_int64), ("gain", c_float * 3), ("offset", c_float * 3),
                ("is_normal", c_int32), ("reserved", c_int32)]


# name -> argtypes (restype is int unless listed in _RESTYPES); must match include/drn.h one-to-one
SIGNATURES = {
    "drn_attention_plan": [_I, _L, _L, POINTER(c_int64)],
    "drn_dit_forward": [POINTER(DitForwardArgs), _P],
    "drn_dit_forward_range": [POINTER(DitForwardArgs), _I, _I, _I, _P],
    "drn_dit_forward_args_bytes": [],
    "drn_dit_sub_bytes": [],
    "drn_dit_forward_gemm_workspace_bytes": [_L, _L, _L, _L, _L, _L],
    "drn_dit_forward_attn_workspace_bytes": [_L, _I, _L],
    "drn_dit_forward_mx_act_bytes": [_L, _L, _L, _L],
    "drn_dit_forward_mx_gemm_workspace_bytes": [_L, _L, _L, _L],
    "drn_dit_forward_mx_u_bytes": [_L, _L, _L],
    "drn_timer_create": [_I, _I],
    "drn_timer_destroy": [_P],
    "drn_timer_count": [_P],
    "drn_timer_seen": [_P, _I],
    "drn_timer_read": [_P, _I, POINTER(c_int), POINTER(c_float), POINTER(c_double), POINTER(c_double)],
    "drn_abi_version": [],
    "drn_error_string": [_I],
    "drn_gemm_bf16": [_P, _P, _P, _L, _L, _L, _L, _L, _L, _I, _P, _P, _L, _L, _P],
    "drn_gemm_bf16_blocked": [_P, _P, _P, _L, _L, _L, _L, _L, _L, _I, _P, _P, _L, _L, _L, _L, _L, _L, _P],
    "drn_gemm_bf16_splitk": [_P, _P, _P, _L, _L, _L, _L, _L, _L, _I, _P, _P, _L, _L, _I, _P, _P],
    "drn_gemm_splitk_workspace_bytes": [_L, _L, _I],
    "drn_gemm_bf16_f32out": [_P, _P, _P, _L, _L, _L, _L, _L, _P],
    "drn_gemm_bf16_splitk_partials": [_P, _P, _L, _L, _L, _L, _L, _L, _I, _P, _P],
    "drn_splitk_gate_res_ln_modulate": [_P, _I, _P, _P, _P, _P, _P, _P, _L, _L, _L, _F, _P],
    "drn_gemm_splitk_choice": [_L, _L, _L],
    "drn_gemm_tile_choice": [_L, _L],
    "drn_gemm_force_tile": [_I],
    "drn_gemm_plan_choice": [_L, _L, _L, _L, _P],
    "drn_gemm_plan_describe": [_L, _L, _L, _L, _L, _L, _L, _I, _L, _L, _L, _I, POINTER(c_int64), _I],
    "drn_gemm_force_res_prefetch": [_I],
    "drn_gemm_tall_force_shape": [_I],
    "drn_mx_quant_bf16": [_P, _L, _L, _L, _P, _P, _P],
    "drn_mx_quant_calls": [_I],
    "drn_gemm_mxfp8_gelu_mx": [_P, _P, _P, _P, _P, _P, _L, _L, _L, _L, _P],
    "drn_ln_modulate_mx": [_P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _F, _P],
    "drn_splitk_gate_res_ln_modulate_mx": [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _F, _P],
    "drn_attention_bf16_mx": [_P, _P, _P, _P, _P, _P, _I, _I, _L, _L, _L, _L, _L, _L, _L, _L, _L, _L, _F, _P],
    "drn_attention_splitkv_bf16_mx": [_P, _P, _P, _P, _P, _P, _I, _I, _L, _L, _L, _L, _L, _L, _L, _L, _L, _L, _F, _I, _P, _P],
    "drn_attention_mx_available": [],
    "drn_attention_mxfp8_params": [POINTER(c_int), POINTER(c_float), POINTER(c_int)],
    "drn_attention_mxfp8_choice": [_I, _L],
    "drn_attention_mxfp8_force": [_I],
    "drn_qk_norm_rope_mx": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _L, _L, _L, _L, _F, _I, _P],
    "drn_mx_quant_vt": [_P, _P, _P, _I, _I, _L, _L, _L, _P],
    "drn_attention_mxfp8": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _L, _L, _L, _L, _L, _L, _F, _P],
    "drn_attention_splitkv_mxfp8": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _L, _L, _L, _L, _L, _L, _F, _I, _P, _P],
    "drn_dit_forward_mx_attn_bytes": [_L, _L, _L],
    "drn_dit_forward_mx_attn_layout": [_L, _L, _L, POINTER(c_int64)],
    "drn_gemm_mxfp8": [_P, _P, _P, _P, _P, _L, _L, _L, _L, _I, _P, _P, _L, _L, _P],
    "drn_gemm_mxfp8_blocked": [_P, _P, _P, _P, _P, _L, _L, _L, _L, _I, _P, _P, _L, _L, _L, _L, _L, _L, _P],
    "drn_gemm_mxfp8_splitk_choice": [_L, _L, _L],
    "drn_gemm_mxfp8_splitk": [_P, _P, _P, _P, _P, _L, _L, _L, _L, _I, _P, _P, _L, _L, _I, _P, _P],
    "drn_gemm_mxfp8_splitk_partials": [_P, _P, _P, _P, _L, _L, _L, _L, _I, _P, _P],
    "drn_gemm_mxfp8_force_small_m": [_I],
    "drn_gemm_mxfp8_tall_force_shape": [_I],
    "drn_gemv_bf16": [_P, _P, _P, _L, _L, _I, _I, _L, _L, _L, _L, _L, _P, _L, _L, _P, _L, _L, _I, _P],
    "drn_ln_modulate": [_P, _P, _P, _P, _P, _L, _L, _L, _F, _P],
    "drn_ln_force_kernel": [_I],
    "drn_bcast_add": [_P, _P, _L, _L, _L, _P],
    "drn_permute_021": [_P, _P, _L, _L, _L, _P],
    "drn_rmsnorm": [_P, _P, _P, _L, _L, _F, _P],
    "drn_qk_norm_rope": [_P, _P, _P, _P, _P, _P, _L, _I, _L, _L, _L, _L, _F, _P],
    "drn_attention_bf16": [_P, _P, _P, _P, _I, _I, _L, _L, _L, _L, _L, _L, _L, _L, _L, _L, _F, _P],
    "drn_attention_splitkv_bf16": [_P, _P, _P, _P, _I, _I, _L, _L, _L, _L, _L, _L, _L, _L, _L, _L, _F, _I, _P, _P],
    "drn_attention_splitkv_workspace_bytes": [_I, _I, _L, _I],
    "drn_attention_force_shape16": [_I],
    "drn_patchify_concat": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _L, _P],
    "drn_unpatchify": [_P, _L, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "drn_edm_scale_input": [_P, _P, _L, _F, _P],
    "drn_edm_step": [_P, _P, _P, _L, _F, _F, _F, _F, _P],
    "drn_cfg_combine": [_P, _P, _P, _L, _F, _P],
    "drn_sampler_step_2m": [_P, _P, _F, _P, _P, _P, _P, _P, _I, _L, _F, _F, _F, _F, _F, _F, _P],
    "drn_ensemble_reduce_u8": [POINTER(c_void_p), _I, _P, _P, _L, _I, _P],
    "drn_ensemble_align_workspace_bytes": [_I, _I, _L],
    "drn_ensemble_align_affine": [POINTER(c_void_p), _I, _I, _L, _P, _P, _P, _L, _P],
    "drn_ensemble_reduce_affine_u8": [POINTER(c_void_p), _I, _P, _I, _L, _P, _P, _I, _P],
    "drn_gbuffer_edit_map_bytes": [],
    "drn_gbuffer_edit_u8": [POINTER(GbufferEditMap), _I, _P, _L, _L, _P, _L, _L, _I, _I, _L, _P],
    "drn_step_cache_workspace_bytes": [_I, _L],
    "drn_step_cache_probe": [_P, _P, _P, _P, _L, _I, _L, _P],
    "drn_step_cache_residual": [_P, _P, _P, _L, _P],
    "drn_step_cache_apply": [_P, _P, _L, _P],
    "drn_postprocess_u8": [_P, _P, _I, _I, _I, _I, _I, _P],
    "drn_postprocess_window_u8": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "drn_window_align_workspace_bytes": [_I, _I, _I, _I],
    "drn_window_align_affine": [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P],
    "drn_postprocess_window_align_u8": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "drn_env_project": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _F, _P],
    "drn_env_cubes": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _I, _P],
    "drn_env_project_seq": [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P],
    "drn_fit_frames": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _I, _P],
    "drn_fit_frames_u8": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _I, _P],
    "drn_restore_frames_u8": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P],
    "drn_restore_guided_u8": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _F, _P],
    "drn_tile_blend_u8": [_P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "drn_latent_tile_gather": [_P, _P, _L, _I, _I, _I, _I, _I, _I, _F, _I, _P],
    "drn_latent_tile_step_join": [_P, _P, _F, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _F, _P],
}
_RESTYPES = {"drn_error_string": c_char_p, "drn_attention_splitkv_workspace_bytes": c_int64,
             "drn_gemm_splitk_workspace_bytes": c_int64, "drn_dit_forward_gemm_workspace_bytes": c_int64,
             "drn_dit_forward_attn_workspace_bytes": c_int64, "drn_dit_forward_mx_act_bytes": c_int64,
             "drn_dit_forward_mx_u_bytes": c_int64, "drn_mx_quant_calls": c_int64, "drn_dit_forward_mx_attn_bytes": c_int64,
             "drn_window_align_workspace_bytes": c_int64, "drn_step_cache_workspace_bytes": c_int64,
             "drn_ensemble_align_workspace_bytes": c_int64,
             "drn_dit_forward_mx_gemm_workspace_bytes": c_int64, "drn_dit_forward_args_bytes": c_int64, "drn_dit_sub_bytes": c_int64, "drn_timer_create": c_void_p, "drn_timer_destroy": None,
             "drn_ln_force_kernel": None, "drn_attention_force_shape16": None}


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def load_library():
    """Load libdrn.so and bind every symbol declared in include/drn.h.  Raises if anything is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                           "there is no CPU / eager fallback for the hot path")
    lib = ctypes.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)
    if lib.drn_abi_version() != 1:
        raise RuntimeError("libdrn.so ABI version mismatch")
    if lib.drn_dit_forward_args_bytes() != ctypes.sizeof(DitForwardArgs) or lib.drn_dit_sub_bytes() != ctypes.sizeof(DitSub):
        raise RuntimeError("libdrn.so: drn_dit_forward_args / drn_dit_sub layout differs from the ctypes mirror in native.py")
    if lib.drn_gbuffer_edit_map_bytes() != ctypes.sizeof(GbufferEditMap):
        raise RuntimeError("libdrn.so: drn_gbuffer_edit_map layout differs from the ctypes mirror in native.py")
    _LIB = lib
    return lib


def _check(code: int, what: str):
    if code != 0:
        msg = load_library().drn_error_string(code)
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else '?'}")


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda, "device tensor required"
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bf16(*ts):
    for t in ts:
        if t is not None:
            assert t.dtype == torch.bfloat16, f"bf16 tensor required, got {t.dtype}"


# ----------------------------------------------------------------------------------------------- kernel timing hook
class KernelTimer:
    """HIP-event timing of individual launches on the launch stream (bench.py's roofline leg).

    torch.cuda.Event records on torch's current stream, which is the stream every wrapper below launches on.
    """

    def __init__(self, names=("gemm", "attention"), sample_every=1):
        """sample_every = n times every n-th launch of each name only (an event pair costs ~35 us of queue time on the
        GPU, ~10 ms per DiT forward if every launch is bracketed); use an n coprime with the launch pattern's period."""
        self.names = set(names)
        self.sample_every = max(1, int(sample_every))
        self.counts = {}
        self.records = []          # (name, start_event, end_event, flops, bytes)
        self._native = None        # drn_timer handle: launches enqueued by drn_dit_forward are bracketed in C

    def native_handle(self, capacity=8192):
        """The event pool drn_dit_forward records into (same sampling rule, kinds 0 = gemm, 1 = attention); None when this
        timer does not watch those kernels."""
        if not ({"gemm", "attention"} <= self.names):
            return None
        if self._native is None:
            h = load_library().drn_timer_create(capacity, self.sample_every)
            if not h:
                raise RuntimeError("drn_timer_create failed")
            self._native = c_void_p(h)
        return self._native

    def __del__(self):
        if getattr(self, "_native", None) is not None and _LIB is not None:
            _LIB.drn_timer_destroy(self._native)
            self._native = None

    def begin(self, name):
        if name not in self.names:
            return None
        c = self.counts.get(name, 0)
        self.counts[name] = c + 1
        if c % self.sample_every:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name, start, flops, nbytes):
        if start is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.records.append((name, start, e, flops, nbytes))

    def summary(self):
        """name -> dict(launches, ms_total, ms_avg, flops, bytes); call after a synchronize."""
        out = {}
        for name, s, e, fl, by in self.records:
            d = out.setdefault(name, {"launches": 0, "ms_total": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms_total"] += s.elapsed_time(e)
            d["flops"] += fl
            d["bytes"] += by
        seen = dict(self.counts)
        if self._native is not None:
            lib = load_library()
            kind, ms, fl, by = c_int(), c_float(), c_double(), c_double()
            for i in range(lib.drn_timer_count(self._native)):
                _check(lib.drn_timer_read(self._native, i, kind, ms, fl, by), "drn_timer_read")
                name = ("gemm", "attention")[kind.value]
                d = out.setdefault(name, {"launches": 0, "ms_total": 0.0, "flops": 0.0, "bytes": 0.0})
                d["launches"] += 1
                d["ms_total"] += ms.value
                d["flops"] += fl.value
                d["bytes"] += by.value
            for k, name in enumerate(("gemm", "attention")):
                seen[name] = seen.get(name, 0) + lib.drn_timer_seen(self._native, k)
        for name, d in out.items():
            d["ms_avg"] = d["ms_total"] / max(d["launches"], 1)
            d["launches_seen"] = seen.get(name, d["launches"])      # all launches, timed or not
        return out


_TIMER = None


def set_timer(t):
    global _TIMER
    _TIMER = t


# ----------------------------------------------------------------------------------------------- wrappers

_SPLIT_WS = {}


def _split_workspace(key, nbytes, grow):
    """The cached device scratch of the split launches (fp32 partials).  grow (the split-K GEMMs, key (device, "gemm")): one buffer
    that only ever grows.  Else (split-KV attention, key (device, nbytes)): a buffer of exactly that size, replacing whatever the
    cache held (one shape is kept resident)."""
    ws = _SPLIT_WS.get(key)
    if ws is None or (grow and ws.numel() < nbytes):
        if not grow:
            _SPLIT_WS.clear()
        ws = torch.empty(nbytes, dtype=torch.uint8, device=key[0])
        _SPLIT_WS[key] = ws
    return ws


def _clip_rows(M, rows_per_batch):
    """The rows of ONE clip: launch decisions that change the summation order come from them, so clips stacked along the rows
    (rows_per_batch) get the plan of a clip alone (batch-invariant results)."""
    rpb = rows_per_batch if rows_per_batch else max(M, 1)
    return rpb if (0 < rpb < M and M % rpb == 0) else M


def gemm(a, w, out=None, epilogue=EPI_NONE, gate=None, residual=None, rows_per_batch=None, splitk=None):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T).  a/w/out may be row-strided 2-D views (last dim contiguous)."""
    _bf16(a, w, out, gate, residual)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.stride(1) == 1 and w.stride(1) == 1
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    ldr = residual.stride(0) if residual is not None else 0
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
    t0 = _TIMER.begin("gemm") if _TIMER is not None else None
    lib = load_library()
    rpb = rows_per_batch if rows_per_batch else max(M, 1)
    Mb = _clip_rows(M, rows_per_batch)
    splits = lib.drn_gemm_splitk_choice(Mb, N, K) if (Mb <= 1024 and splitk is None) else (splitk or 1)
    if splits > 1:
        # few tokens: the product streams the weights; K is split over several workgroups per tile to keep the CUs busy
        ws = _split_workspace((a.device, "gemm"), lib.drn_gemm_splitk_workspace_bytes(M, N, splits), grow=True)
        _check(lib.drn_gemm_bf16_splitk(_ptr(a), _ptr(w), _ptr(out), M, N, K, a.stride(0), w.stride(0), out.stride(0), epilogue,
                                        _ptr(gate), _ptr(residual), ldr, rpb, splits, ws.data_ptr(), _stream()),
               "drn_gemm_bf16_splitk")
    else:
        _check(lib.drn_gemm_bf16(_ptr(a), _ptr(w), _ptr(out), M, N, K, a.stride(0), w.stride(0), out.stride(0),
                                 epilogue, _ptr(gate), _ptr(residual), ldr, rpb, _stream()), "drn_gemm_bf16")
    if t0 is not None:
        _TIMER.end("gemm", t0, 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N * (2 if residual is not None else 1)))
    return out


def gemm_blocked_ok(M, N) -> bool:
    """True when gemm_blocked can run an [M, N] output (every tile kernel but the 128x128 one has the blocked layouts)."""
    return load_library().drn_gemm_tile_choice(M, N) != 0


def gemm_blocked(a, w, out, M, epilogue=EPI_NONE, gate=None, residual=None, a_planes=False, c_planes=False):
    """epi(A @ w^T) with A and / or C stored as planes of columns (drn_gemm_bf16_blocked).
    a_planes: `a` is [P, M, Kb] contiguous = logical A[M, P*Kb] (plane p holds columns p*Kb ..);
    c_planes: `out` is [P, M, Nb] contiguous = logical C[M, P*Nb].  Otherwise plain [M, K] / [M, N] row-strided views."""
    _bf16(a, w, out, gate, residual)
    N, K = w.shape
    assert w.stride(1) == 1
    if a_planes:
        P, Ma, Kb = a.shape
        assert a.is_contiguous() and Ma == M and P * Kb == K
        lda, abc, abs_ = Kb, Kb, M * Kb
    else:
        assert a.shape == (M, K) and a.stride(1) == 1
        lda, abc, abs_ = a.stride(0), 0, 0
    if c_planes:
        P, Mc, Nb = out.shape
        assert out.is_contiguous() and Mc == M and P * Nb == N
        ldc, cbc, cbs = Nb, Nb, M * Nb
    else:
        assert out.shape == (M, N) and out.stride(1) == 1
        ldc, cbc, cbs = out.stride(0), 0, 0
    ldr = residual.stride(0) if residual is not None else 0
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
    t0 = _TIMER.begin("gemm") if _TIMER is not None else None
    _check(load_library().drn_gemm_bf16_blocked(_ptr(a), _ptr(w), _ptr(out), M, N, K, lda, w.stride(0), ldc, epilogue,
                                                _ptr(gate), _ptr(residual), ldr, max(M, 1), abc, abs_, cbc, cbs, _stream()),
           "drn_gemm_bf16_blocked")
    if t0 is not None:
        _TIMER.end("gemm", t0, 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N * (2 if residual is not None else 1)))
    return out


class MxTensor:
    """An MXFP8 matrix (drn.h, MXFP8 block linears): q [rows, K] e4m3fn, scales [rows, K / 32] uint8 (E8M0 bytes)."""

    def __init__(self, q, scales):
        self.q, self.scales = q, scales

    @property
    def shape(self):
        return self.q.shape


def mx_quant(x, out=None):
    """bf16 [M, K] (row-strided view allowed) -> MxTensor, on the device (drn_mx_quant_bf16).  `out`: an MxTensor to reuse."""
    _bf16(x)
    M, K = x.shape
    assert x.stride(1) == 1
    if K % 32:
        raise ValueError(f"MXFP8 quantisation needs K % 32 == 0 (K = {K})")
    if out is None:
        out = MxTensor(torch.empty((M, K), dtype=torch.float8_e4m3fn, device=x.device),
                       torch.empty((M, K // 32), dtype=torch.uint8, device=x.device))
    assert out.q.shape == (M, K) and out.q.is_contiguous() and out.scales.shape == (M, K // 32) and out.scales.is_contiguous()
    _check(load_library().drn_mx_quant_bf16(_ptr(x), M, K, x.stride(0), _ptr(out.q), _ptr(out.scales), _stream()),
           "drn_mx_quant_bf16")
    return out


def mx_empty(M, K, device) -> MxTensor:
    """An uninitialised MxTensor [M, K] (K % 32 == 0): the `out_mx` of a fused producer."""
    if K % 32:
        raise ValueError(f"MXFP8 needs K % 32 == 0 (K = {K})")
    return MxTensor(torch.empty((M, K), dtype=torch.float8_e4m3fn, device=device),
                    torch.empty((M, K // 32), dtype=torch.uint8, device=device))


def _mx_out(out_mx, M, K, device) -> MxTensor:
    """out_mx=True -> a fresh MxTensor; an MxTensor -> checked and reused."""
    if out_mx is True:
        return mx_empty(M, K, device)
    assert isinstance(out_mx, MxTensor) and out_mx.q.shape == (M, K) and out_mx.q.is_contiguous()
    assert out_mx.scales.shape == (M, K // 32) and out_mx.scales.is_contiguous()
    return out_mx


def mx_quant_calls(reset=False) -> int:
    """Launches drn_mx_quant_bf16 has enqueued in this process so far (reset=True zeroes the counter after reading)."""
    return int(load_library().drn_mx_quant_calls(1 if reset else 0))


def attention_mx_available() -> bool:
    """True when attention(..., out_mx=) has a kernel: the 16x16x32 body is selected (drn.h)."""
    return bool(load_library().drn_attention_mx_available())


def mx_gemm_plan(M, N, K, rows_per_batch=None) -> int:
    """How gemm_mxfp8 runs an [M, N, K] product: 0 = drn_gemm_mxfp8 (256 x 256 tiles), s >= 1 = the few-token kernel with s K
    slices (1 = unsplit, fused epilogue).  Decided by drn_gemm_mxfp8_splitk_choice from ONE clip's rows (_clip_rows).  Host-only."""
    return int(load_library().drn_gemm_mxfp8_splitk_choice(_clip_rows(M, rows_per_batch), N, K))


def gemm_mxfp8(a, w, out=None, epilogue=EPI_NONE, gate=None, residual=None, rows_per_batch=None, splitk=None, out_mx=None):
    """out[M, N] = epi(dequant(a) @ dequant(w)^T) for MxTensors a [M, K], w [N, K].  N % 256 == 0, K % 128 == 0.
    splitk: None = mx_gemm_plan decides (drn_gemm_mxfp8, or the few-token kernel drn_gemm_mxfp8_splitk with its K slices);
    0 = drn_gemm_mxfp8; k >= 1 = the few-token kernel with k slices.
    out_mx (True or an MxTensor [M, N]; epilogue EPI_GELU, splitk None): the result leaves as MXFP8 - the bytes of
    mx_quant(out) - and that MxTensor is returned; no bf16 output is written (drn_gemm_mxfp8_gelu_mx).  Raises where the plan
    slices K (mx_gemm_plan > 1): there the GELU lives in the reduce launch."""
    _bf16(out, gate, residual)
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"MXFP8 GEMM: K of a ({K}) and w ({w.shape[1]}) differ")
    if N % 256 or K % 128:
        raise ValueError(f"MXFP8 GEMM needs N % 256 == 0 and K % 128 == 0 (N = {N}, K = {K})")
    if out_mx is not None:
        if epilogue != EPI_GELU or splitk is not None or out is not None:
            raise ValueError("gemm_mxfp8(out_mx=) is the GELU epilogue under the automatic plan, without a bf16 output")
        if mx_gemm_plan(M, N, K, rows_per_batch) > 1:
            raise ValueError(f"gemm_mxfp8(out_mx=): the plan slices K at M={M} N={N} K={K} (no MX epilogue in the reduce launch)")
        out_mx = _mx_out(out_mx, M, N, a.q.device)
        t0 = _TIMER.begin("gemm") if _TIMER is not None else None
        _check(load_library().drn_gemm_mxfp8_gelu_mx(_ptr(a.q), _ptr(a.scales), _ptr(w.q), _ptr(w.scales), _ptr(out_mx.q),
                                                     _ptr(out_mx.scales), M, N, K, rows_per_batch if rows_per_batch else max(M, 1),
                                                     _stream()), "drn_gemm_mxfp8_gelu_mx")
        if t0 is not None:
            _TIMER.end("gemm", t0, 2.0 * M * N * K, 1.03 * (M * K + N * K + M * N))
        return out_mx
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.q.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    ldr = residual.stride(0) if residual is not None else 0
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
    t0 = _TIMER.begin("gemm") if _TIMER is not None else None
    rpb = rows_per_batch if rows_per_batch else max(M, 1)
    lib = load_library()
    splits = mx_gemm_plan(M, N, K, rows_per_batch) if splitk is None else int(splitk)
    if splits >= 1:
        ws = None
        if splits > 1:
            ws = _split_workspace((a.q.device, "gemm"), lib.drn_gemm_splitk_workspace_bytes(M, N, splits), grow=True)
        _check(lib.drn_gemm_mxfp8_splitk(_ptr(a.q), _ptr(a.scales), _ptr(w.q), _ptr(w.scales), _ptr(out), M, N, K, out.stride(0),
                                         epilogue, _ptr(gate), _ptr(residual), ldr, rpb, splits, _ptr(ws), _stream()),
               "drn_gemm_mxfp8_splitk")
    else:
        _check(lib.drn_gemm_mxfp8(_ptr(a.q), _ptr(a.scales), _ptr(w.q), _ptr(w.scales), _ptr(out), M, N, K, out.stride(0),
                                  epilogue, _ptr(gate), _ptr(residual), ldr, rpb, _stream()), "drn_gemm_mxfp8")
    if t0 is not None:
        _TIMER.end("gemm", t0, 2.0 * M * N * K, 1.03 * (M * K + N * K) + 2.0 * M * N * (2 if residual is not None else 1))
    return out


def mx_plane_args(planes):
    """(block_cols, row stride, block_stride) of a tensor of column planes [P, M, cols] as drn_gemm_mxfp8_blocked takes them: plane p
    holds the logical columns p * cols .. of every row; the planes may be views of wider allocations (rows past M behind each
    plane), the columns of a row are contiguous.  Strides in elements of the tensor.  Host-only (any device, meta included)."""
    P, M, cols = planes.shape
    assert planes.stride(2) == 1 and planes.stride(1) >= cols
    return cols, planes.stride(1), planes.stride(0) if P > 1 else max(planes.stride(0), M * planes.stride(1))


def gemm_mxfp8_blocked(a, w, out, M, epilogue=EPI_NONE, gate=None, residual=None, a_planes=False, c_planes=False):
    """gemm_mxfp8 with A and / or C stored as planes of columns (drn_gemm_mxfp8_blocked; always the 256 x 256 kernel).
    a_planes: `a` is an MxTensor with q [P, M, Kb] = logical A[M, P*Kb] (plane p holds columns p*Kb ..; rows contiguous) and scales
    [P, M, Kb/32], planes q.stride(0) bytes resp. q.stride(0) / 32 scale bytes apart; c_planes: `out` is bf16 [P, M, Nb] = logical
    C[M, P*Nb].  Otherwise a plain MxTensor [M, K] / a row-strided [M, N] view.  The residual stays plain."""
    _bf16(out, gate, residual)
    N, K = w.shape
    if a_planes:
        P, Ma, Kb = a.q.shape
        abc, lda, abs_ = mx_plane_args(a.q)
        sbc, lds, sbs = mx_plane_args(a.scales)
        assert Ma == M and P * Kb == K and lda == Kb and a.scales.shape == (P, M, Kb // 32) and lds == Kb // 32 and sbs * 32 == abs_
    else:
        assert a.q.shape == (M, K) and a.q.is_contiguous() and a.scales.shape == (M, K // 32) and a.scales.is_contiguous()
        abc, abs_ = 0, 0
    if c_planes:
        P, Mc, Nb = out.shape
        cbc, ldc, cbs = mx_plane_args(out)
        assert Mc == M and P * Nb == N
    else:
        assert out.shape == (M, N) and out.stride(1) == 1
        ldc, cbc, cbs = out.stride(0), 0, 0
    ldr = residual.stride(0) if residual is not None else 0
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
    t0 = _TIMER.begin("gemm") if _TIMER is not None else None
    _check(load_library().drn_gemm_mxfp8_blocked(_ptr(a.q), _ptr(a.scales), _ptr(w.q), _ptr(w.scales), _ptr(out), M, N, K, ldc,
                                                 epilogue, _ptr(gate), _ptr(residual), ldr, max(M, 1), abc, abs_, cbc, cbs,
                                                 _stream()), "drn_gemm_mxfp8_blocked")
    if t0 is not None:
        _TIMER.end("gemm", t0, 2.0 * M * N * K, 1.03 * (M * K + N * K) + 2.0 * M * N * (2 if residual is not None else 1))
    return out


def gemv(x, w, out=None, add=None, mul=None, act=ACT_NONE):
    """Grouped batch-1 GEMV.  x: [G|1, B, K]; w: [G, N, K]; out/add/mul: [G, B, N] (add/mul may have G == 1)."""
    _bf16(x, w, out, add, mul)
    G, N, K = w.shape
    assert x.dim() == 3 and x.shape[2] == K and x.is_contiguous() and w.is_contiguous()
    B = x.shape[1]
    if out is None:
        out = torch.empty((G, B, N), dtype=torch.bfloat16, device=x.device)
    assert out.shape == (G, B, N) and out.is_contiguous()

    def gs(t, inner):
        if t is None:
            return 0, 0
        assert t.is_contiguous() and t.dim() == 3 and t.shape[1] == B and t.shape[2] == inner
        return (0 if t.shape[0] == 1 else B * inner), inner

    xg, xb = gs(x, K)
    ag, ab = gs(add, N)
    mg, mb = gs(mul, N)
    _check(load_library().drn_gemv_bf16(_ptr(x), _ptr(w), _ptr(out), N, K, G, B, xg, xb, N * K, B * N, N,
                                        _ptr(add), ag, ab, _ptr(mul), mg, mb, act, _stream()), "drn_gemv_bf16")
    return out


def ln_modulate(x, shift, scale, out=None, add_vec=None, rows_per_batch=None, eps=1e-6, out_mx=None):
    """out = bf16(bf16(LN(x) * bf16(1+scale)) + shift); if add_vec: x <- bf16(x + add_vec) in place first.
    out_mx (True or an MxTensor [rows, D]): the result leaves as MXFP8 - the bytes of mx_quant(out) - and that MxTensor is
    returned; the bf16 `out` is written as well only when given (drn_ln_modulate_mx)."""
    _bf16(x, shift, scale, out, add_vec)
    rows, D = x.shape
    assert x.is_contiguous()
    if out_mx is not None:
        out_mx = _mx_out(out_mx, rows, D, x.device)
        assert out is None or (out.shape == x.shape and out.is_contiguous())
        _check(load_library().drn_ln_modulate_mx(_ptr(x), _ptr(add_vec), _ptr(shift), _ptr(scale), _ptr(out), _ptr(out_mx.q),
                                                 _ptr(out_mx.scales), rows, D, rows_per_batch if rows_per_batch else max(rows, 1),
                                                 eps, _stream()), "drn_ln_modulate_mx")
        return out_mx
    if out is None:
        out = torch.empty_like(x)
    _check(load_library().drn_ln_modulate(_ptr(x), _ptr(add_vec), _ptr(shift), _ptr(scale), _ptr(out), rows, D,
                                          rows_per_batch if rows_per_batch else max(rows, 1), eps, _stream()),
           "drn_ln_modulate")
    return out


def bcast_add(x, vec, rows_per_batch=None):
    _bf16(x, vec)
    rows, D = x.shape
    assert x.is_contiguous()
    _check(load_library().drn_bcast_add(_ptr(x), _ptr(vec), rows, D, rows_per_batch if rows_per_batch else max(rows, 1),
                                        _stream()), "drn_bcast_add")
    return x


def permute_021(x, out=None):
    """[A, B, C] -> [B, A, C] (contiguous both sides)."""
    _bf16(x, out)
    A, B, C = x.shape
    assert x.is_contiguous()
    if out is None:
        out = torch.empty((B, A, C), dtype=torch.bfloat16, device=x.device)
    assert out.is_contiguous() and out.numel() == x.numel()
    _check(load_library().drn_permute_021(_ptr(x), _ptr(out), A, B, C, _stream()), "drn_permute_021")
    return out


def rmsnorm(x, w, eps=1e-6):
    _bf16(x, w)
    rows, D = x.shape
    out = torch.empty_like(x)
    _check(load_library().drn_rmsnorm(_ptr(x), _ptr(w), _ptr(out), rows, D, eps, _stream()), "drn_rmsnorm")
    return out


def qk_norm_rope(q, k, wq, wk, cos, sin, heads, tokens_per_batch=None, pos_offset=0, eps=1e-6):
    """In place on q and/or k: [tokens, heads*128] views with their own row strides; either may be None."""
    _bf16(q, k, wq, wk, cos, sin)
    ref = q if q is not None else k
    tokens = ref.shape[0]
    for t in (q, k):
        if t is not None:
            assert t.shape == (tokens, heads * 128) and t.stride(1) == 1
    _check(load_library().drn_qk_norm_rope(_ptr(q), _ptr(k), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin), tokens, heads,
                                           q.stride(0) if q is not None else 0, k.stride(0) if k is not None else 0,
                                           tokens_per_batch if tokens_per_batch else max(tokens, 1),
                                           pos_offset, eps, _stream()), "drn_qk_norm_rope")


_NUM_CUS = 256          # MI355X


def attention_plan(batch, heads, Sq, Sk):
    """How to cover the (q-block, head) grid of ONE clip with whole rounds of the 256 CUs: a list of (q_begin, q_end, kv_splits)
    from drn_attention_plan (csrc/dit_forward.hip: the same plan drn_dit_forward uses).  The q-blocks that fill whole rounds run
    unsplit; a fractional last round runs as a second launch with its keys cut into chunks (split-KV + combine).  `batch` is
    ignored on purpose: the plan of one clip applies to every clip of a batch (batch-invariant summation order)."""
    buf = (c_int64 * 6)()
    n = load_library().drn_attention_plan(heads, Sq, Sk, buf)
    if n <= 0:
        raise ValueError(f"no attention plan for heads={heads} Sq={Sq} Sk={Sk}")
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(n)]


def _attention_tail(launch, B, H, Sq, Sk, device, out, out_mx, scale, kv_splits, byte_factor):
    """What attention() and attention_mxfp8() share once the operands are checked: the out / out_mx geometry, the walk of the
    plan, the split-KV workspace and the timer.  launch(q0, n, o, oq, os, ldo, bso, scale, extra) enqueues the queries
    [q0, q0 + n) of every clip: o / oq / os are the output pointers advanced to q0 (None = not written), extra = (nsplit, workspace)
    for a launch with split keys, else ()."""
    HD = H * 128
    mx = None
    if out_mx is not None:
        mx = _mx_out(out_mx, B * Sq, HD, device)
        assert out is None or (out.shape == (B, Sq, HD) and out.is_contiguous())
        oq, osc = mx.q.view(B, Sq, HD), mx.scales.view(B, Sq, HD // 32)
        ldo, bso = HD, Sq * HD                 # the MX rows are contiguous; o (optional) must share that geometry
    else:
        if out is None:
            out = torch.empty((B, Sq, HD), dtype=torch.bfloat16, device=device)
        ldo, bso = out.stride(1), out.stride(0)
    if scale is None:
        scale = 1.0 / (128 ** 0.5)
    # the plan of ONE clip, applied to every clip of the batch: a split of the keys changes the summation order, so it must not
    # depend on how many clips are stepped together
    plan = attention_plan(1, H, Sq, Sk) if kv_splits is None else [(0, Sq, int(kv_splits))]
    t0 = _TIMER.begin("attention") if _TIMER is not None else None
    lib = load_library()
    for q0, q1, ns in plan:
        extra = ()
        if ns > 1:
            nbytes = lib.drn_attention_splitkv_workspace_bytes(B, H, q1 - q0, ns)
            extra = (ns, _split_workspace((device, nbytes), nbytes, grow=False).data_ptr())
        launch(q0, q1 - q0, _ptr(out[:, q0:q1]) if out is not None else None, _ptr(oq[:, q0:q1]) if mx is not None else None,
               _ptr(osc[:, q0:q1]) if mx is not None else None, ldo, bso, scale, extra)
    if t0 is not None:
        _TIMER.end("attention", t0, 4.0 * B * H * Sq * Sk * 128, byte_factor * B * H * 128 * (2 * Sq + 2 * Sk))
    return out if mx is None else mx


def attention(q, k, v, out=None, heads=None, scale=None, kv_splits=None, out_mx=None):
    """q: [B, Sq, H*128], k/v: [B, Sk, H*128] (token-strided views allowed) -> out [B, Sq, H*128].
    kv_splits: None = automatic (attention_plan), 1 = single pass, n > 1 = split-KV + combine.
    out_mx (True or an MxTensor [B * Sq, H*128]): the output leaves as MXFP8 - the bytes of mx_quant(out.view(B * Sq, -1)) - and
    that MxTensor is returned; the bf16 `out` (contiguous) is written as well only when given.  Needs attention_mx_available()."""
    _bf16(q, k, v, out)
    B, Sq, HD = q.shape
    Sk = k.shape[1]
    H = heads if heads else HD // 128
    assert HD == H * 128 and q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    if out_mx is not None and not attention_mx_available():
        raise RuntimeError("attention(out_mx=): the 32x32x16 body is selected and has no MX epilogue (drn.h)")
    lib = load_library()

    def launch(q0, n, o, oq, osc, ldo, bso, scale, extra):
        # (o [, oq, os]): the _mx entries take the two MX pointers behind o, everything else is the same call
        name = "drn_attention" + ("_splitkv" if extra else "") + "_bf16" + ("_mx" if oq is not None else "")
        outs = (o,) if oq is None else (o, oq, osc)
        _check(getattr(lib, name)(_ptr(q[:, q0:q0 + n]), _ptr(k), _ptr(v), *outs, B, H, n, Sk, q.stride(1), k.stride(1), v.stride(1),
                                  ldo, q.stride(0), k.stride(0), v.stride(0), bso, scale, *extra, _stream()), name)

    return _attention_tail(launch, B, H, Sq, Sk, q.device, out, out_mx, scale, kv_splits, 2.0)


# ----------------------------------------------------------------------------------------------- MXFP8 self-attention
def attention_mxfp8_params():
    """(key_tile, rescale_thr, pexp) of the MXFP8 attention kernel as built (drn_attention_mxfp8_params; host-only)."""
    kt, thr, pe = c_int(), c_float(), c_int()
    _check(load_library().drn_attention_mxfp8_params(kt, thr, pe), "drn_attention_mxfp8_params")
    return kt.value, thr.value, pe.value


def attention_mxfp8_choice(heads, S) -> bool:
    """Whether a self-attention site of S tokens per clip runs on the MXFP8 kernels when the switch is on (drn_attention_mxfp8_choice:
    the rule drn_dit_forward applies; host-only)."""
    return bool(load_library().drn_attention_mxfp8_choice(heads, S))


def attention_mxfp8_force(on: int) -> int:
    """1 = every site of an engine with the switch on takes the MXFP8 kernels, 0 = the measured rule (default); returns the
    previous setting (tests / A-B runs)."""
    return int(load_library().drn_attention_mxfp8_force(on))


def qk_norm_rope_mx(q, k, wq, wk, cos, sin, heads, tokens_per_batch=None, pos_offset=0, eps=1e-6, write_bf16=False,
                    out_q=None, out_k=None):
    """qk_norm_rope with the result written as MXFP8: returns (MxTensor of q or None, MxTensor of k or None), contiguous
    [tokens, heads*128]; the in-place bf16 result is written as well only with write_bf16 (drn_qk_norm_rope_mx)."""
    _bf16(q, k, wq, wk, cos, sin)
    ref = q if q is not None else k
    tokens = ref.shape[0]
    for t in (q, k):
        if t is not None:
            assert t.shape == (tokens, heads * 128) and t.stride(1) == 1
    mq = _mx_out(out_q if out_q is not None else True, tokens, heads * 128, ref.device) if q is not None else None
    mk = _mx_out(out_k if out_k is not None else True, tokens, heads * 128, ref.device) if k is not None else None
    _check(load_library().drn_qk_norm_rope_mx(_ptr(q), _ptr(k), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin),
                                              _ptr(mq.q) if mq else None, _ptr(mq.scales) if mq else None,
                                              _ptr(mk.q) if mk else None, _ptr(mk.scales) if mk else None, tokens, heads,
                                              q.stride(0) if q is not None else 0, k.stride(0) if k is not None else 0,
                                              tokens_per_batch if tokens_per_batch else max(tokens, 1), pos_offset, eps,
                                              1 if write_bf16 else 0, _stream()), "drn_qk_norm_rope_mx")
    return mq, mk


def mx_quant_vt(v, heads=None, out=None):
    """v [B, Sk, H*128] bf16 (token- / batch-strided view allowed) -> (vt [B, H, 128, Skp] e4m3, vs [B, H, 128, Skp/32] uint8): V
    transposed and quantised along the keys, zero-padded to Skp = Sk rounded up to 128 (drn_mx_quant_vt).  out: a (vt, vs) pair."""
    _bf16(v)
    B, Sk, HD = v.shape
    H = heads if heads else HD // 128
    assert HD == H * 128 and v.stride(2) == 1
    Skp = (Sk + 127) // 128 * 128
    if out is None:
        out = (torch.empty((B, H, 128, Skp), dtype=torch.float8_e4m3fn, device=v.device),
               torch.empty((B, H, 128, Skp // 32), dtype=torch.uint8, device=v.device))
    vt, vs = out
    assert vt.shape == (B, H, 128, Skp) and vt.is_contiguous() and vs.shape == (B, H, 128, Skp // 32) and vs.is_contiguous()
    _check(load_library().drn_mx_quant_vt(_ptr(v), _ptr(vt), _ptr(vs), B, H, Sk, v.stride(1), v.stride(0), _stream()),
           "drn_mx_quant_vt")
    return vt, vs


def attention_mxfp8(qm, km, vt, vs, B, Sq, Sk, q_bs=None, k_bs=None, out=None, scale=None, kv_splits=None, out_mx=None):
    """MXFP8 attention (drn_attention_mxfp8 / drn_attention_splitkv_mxfp8).  qm / km: MxTensors [rows, H*128] with clip b's queries
    from row b * q_bs (default Sq) and keys from row b * k_bs (default Sk); vt / vs from mx_quant_vt for (B, H, Sk).
    -> out [B, Sq, H*128] bf16, or with out_mx (True or an MxTensor [B * Sq, H*128]) that MxTensor (bf16 `out` only when given).
    kv_splits as attention()."""
    _bf16(out)
    HD = qm.q.shape[1]
    H = HD // 128
    q_bs = Sq if q_bs is None else q_bs
    k_bs = Sk if k_bs is None else k_bs
    Skp = (Sk + 127) // 128 * 128
    assert HD == H * 128 and km.q.shape[1] == HD and qm.q.is_contiguous() and km.q.is_contiguous()
    assert qm.q.shape[0] >= (B - 1) * q_bs + Sq and km.q.shape[0] >= (B - 1) * k_bs + Sk
    assert vt.shape == (B, H, 128, Skp) and vt.is_contiguous() and vs.shape == (B, H, 128, Skp // 32) and vs.is_contiguous()
    lib = load_library()

    def launch(q0, n, o, oq, osc, ldo, bso, scale, extra):
        name = "drn_attention_splitkv_mxfp8" if extra else "drn_attention_mxfp8"
        _check(getattr(lib, name)(_ptr(qm.q[q0:]), _ptr(qm.scales[q0:]), _ptr(km.q), _ptr(km.scales), _ptr(vt), _ptr(vs), o, oq, osc,
                                  B, H, n, Sk, q_bs, k_bs, ldo, bso, scale, *extra, _stream()), name)

    return _attention_tail(launch, B, H, Sq, Sk, qm.q.device, out, out_mx, scale, kv_splits, 1.0)


def patchify_concat(x, cond, with_mask, pt, ps, ldo):
    _bf16(x, cond)
    B, Cx, T, H, W = x.shape
    Cc = cond.shape[1] if cond is not None else 0
    assert x.is_contiguous() and (cond is None or cond.is_contiguous())
    rows = B * (T // pt) * (H // ps) * (W // ps)
    out = torch.empty((rows, ldo), dtype=torch.bfloat16, device=x.device)
    _check(load_library().drn_patchify_concat(_ptr(x), _ptr(cond), _ptr(out), B, Cx, Cc, 1 if with_mask else 0, T, H, W,
                                              pt, ps, ldo, _stream()), "drn_patchify_concat")
    return out


def unpatchify(y, B, C, Tp, Hp, Wp, pt, ps):
    _bf16(y)
    assert y.stride(1) == 1
    out = torch.empty((B, C, Tp * pt, Hp * ps, Wp * ps), dtype=torch.bfloat16, device=y.device)
    _check(load_library().drn_unpatchify(_ptr(y), y.stride(0), _ptr(out), B, C, Tp, Hp, Wp, pt, ps, _stream()),
           "drn_unpatchify")
    return out


def edm_scale_input(x, c_in: float):
    _bf16(x)
    assert x.is_contiguous()
    out = torch.empty_like(x)
    _check(load_library().drn_edm_scale_input(_ptr(x), _ptr(out), x.numel(), c_in, _stream()), "drn_edm_scale_input")
    return out


def edm_step(model_out, sample, c_skip: float, c_out: float, sigma: float, dt: float):
    _bf16(model_out, sample)
    assert model_out.is_contiguous() and sample.is_contiguous() and model_out.numel() == sample.numel()
    out = torch.empty_like(sample)
    _check(load_library().drn_edm_step(_ptr(model_out), _ptr(sample), _ptr(out), sample.numel(), c_skip, c_out, sigma, dt,
                                       _stream()), "drn_edm_step")
    return out


def cfg_combine(cond, uncond, guidance: float):
    _bf16(cond, uncond)
    assert cond.is_contiguous() and uncond.is_contiguous()
    out = torch.empty_like(cond)
    _check(load_library().drn_cfg_combine(_ptr(cond), _ptr(uncond), _ptr(out), cond.numel(), guidance, _stream()),
           "drn_cfg_combine")
    return out


def sampler_step_2m(cond, uncond, guidance: float, x, hist_in, hist_out, c_skip: float, c_out: float, a: float, b1: float,
                    b0: float, c_in_next=None, copies: int = 1):
    """One DPM-Solver++(2M) step in one launch (drn_sampler_step_2m; the plan and the specification: sampler.plan_steps /
    step_reference).  cond (and uncond, or None for no CFG) and x bf16 of one shape [P, ...]; hist_in fp32 of that shape, or None
    where the step reads no history; hist_out fp32 of that shape, written with the denoised estimate (it may be hist_in).  All on
    one device, contiguous.  -> (the new latent, bf16 like x; the next step's model input bf16 [copies * P, ...] = the new latent
    times c_in_next, `copies` (1, or 2 under CFG) times along the batch - or None where c_in_next is None, the last step)."""
    _bf16(cond, uncond, x)
    for name, t in (("cond", cond), ("uncond", uncond), ("x", x), ("hist_in", hist_in), ("hist_out", hist_out)):
        if t is not None:
            assert t.is_contiguous() and t.numel() == x.numel() and t.device == x.device, \
                f"{name}: a contiguous tensor of x's size on x's device required"
    for name, t in (("hist_in", hist_in), ("hist_out", hist_out)):
        assert t is None or t.dtype == torch.float32, f"{name}: the history is fp32"
    assert hist_out is not None, "hist_out: the step always writes its denoised estimate"
    x_out = torch.empty_like(x)
    scaled = None
    if c_in_next is not None:
        scaled = torch.empty((copies * x.shape[0], *x.shape[1:]), dtype=torch.bfloat16, device=x.device)
    _check(load_library().drn_sampler_step_2m(_ptr(cond), _ptr(uncond), guidance, _ptr(x), _ptr(hist_in), _ptr(hist_out),
                                              _ptr(x_out), _ptr(scaled), copies, x.numel(), c_skip, c_out, a, b1, b0,
                                              0.0 if c_in_next is None else c_in_next, _stream()), "drn_sampler_step_2m")
    return x_out, scaled


def postprocess_u8(video, normalize_normal: bool):
    """video [B,3,T,H,W] bf16 -> uint8 [B,T,H,W,3]."""
    _bf16(video)
    B, C, T, H, W = video.shape
    assert C == 3 and video.is_contiguous()
    out = torch.empty((B, T, H, W, 3), dtype=torch.uint8, device=video.device)
    _check(load_library().drn_postprocess_u8(_ptr(video), _ptr(out), B, T, H, W, 1 if normalize_normal else 0, _stream()),
           "drn_postprocess_u8")
    return out


def postprocess_window_u8(video, prev_tail, ramp_w, ramp_at: int, write_lo: int, write_hi: int, normalize_normal: bool, out=None):
    """One window of a long clip (drn_postprocess_window_u8): video [B,3,Tw,H,W] bf16, frames [write_lo, write_hi) -> uint8
    [B, write_hi - write_lo, H, W, 3]; with prev_tail [B,3,O,H,W] bf16 (the previous window's last O decoded frames) and ramp_w
    [O] fp32 on the device, frames [ramp_at, ramp_at + O) are cross-faded first.  prev_tail = ramp_w = None: no ramp."""
    _bf16(video, prev_tail)
    B, C, Tw, H, W = video.shape
    assert C == 3 and video.is_contiguous()
    assert (prev_tail is None) == (ramp_w is None), "prev_tail and ramp_w come together"
    O = 0
    if prev_tail is not None:
        O = prev_tail.shape[2]
        assert prev_tail.shape == (B, 3, O, H, W) and prev_tail.is_contiguous()
        assert ramp_w.dtype == torch.float32 and ramp_w.shape == (O,) and ramp_w.is_contiguous()
    shape = (B, max(write_hi - write_lo, 0), H, W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=video.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()
    _check(load_library().drn_postprocess_window_u8(_ptr(video), _ptr(prev_tail), _ptr(ramp_w), _ptr(out), B, Tw, H, W, O, ramp_at,
                                                    write_lo, write_hi, 1 if normalize_normal else 0, _stream()),
           "drn_postprocess_window_u8")
    return out


def window_align_affine(video, prev_tail, ramp_at: int, moments: bool = False):
    """The gain and offset that match one window to the previous window's carry over the overlap (drn_window_align_affine; the
    specification: windows.align_affine).  video [B,3,Tw,H,W] bf16, prev_tail [B,3,O,H,W] bf16, O >= 1 -> affine [B,2] fp32 =
    (g, o) on the device, never read by the host; with moments=True also the fp64 moments [B,6] behind it."""
    _bf16(video, prev_tail)
    B, C, Tw, H, W = video.shape
    O = prev_tail.shape[2]
    assert C == 3 and video.is_contiguous() and prev_tail.shape == (B, 3, O, H, W) and prev_tail.is_contiguous()
    lib = load_library()
    nbytes = lib.drn_window_align_workspace_bytes(B, H, W, O)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=video.device)
    affine = torch.empty((B, 2), dtype=torch.float32, device=video.device)
    mom = torch.empty((B, 6), dtype=torch.float64, device=video.device) if moments else None
    _check(lib.drn_window_align_affine(_ptr(video), _ptr(prev_tail), _ptr(affine), _ptr(mom), _ptr(ws), nbytes, B, Tw, H, W, O,
                                       ramp_at, _stream()), "drn_window_align_affine")
    return (affine, mom) if moments else affine


def postprocess_window_align_u8(video, prev_tail, ramp_w, affine, ramp_at: int, write_lo: int, write_hi: int,
                                normalize_normal: bool, carry_frames: int = 0, out=None, carry_out=None):
    """postprocess_window_u8 with the affine of window_align_affine ([B,2] fp32 on the device, or None) applied to every window
    value in front of the cross-fade, and (carry_frames = O >= 1, or a carry_out given) the aligned last O frames written as the
    next carry [B,3,O,H,W] bf16 by the same launch (drn_postprocess_window_align_u8) -> (uint8 frames, carry or None)."""
    _bf16(video, prev_tail, carry_out)
    B, C, Tw, H, W = video.shape
    assert C == 3 and video.is_contiguous()
    assert (prev_tail is None) == (ramp_w is None), "prev_tail and ramp_w come together"
    O = int(carry_out.shape[2]) if carry_out is not None else int(carry_frames)
    if prev_tail is not None:
        assert not O or O == prev_tail.shape[2], "the carry written has the length of the carry read"
        O = prev_tail.shape[2]
        assert prev_tail.shape == (B, 3, O, H, W) and prev_tail.is_contiguous()
        assert ramp_w.dtype == torch.float32 and ramp_w.shape == (O,) and ramp_w.is_contiguous()
    if affine is not None:
        assert affine.dtype == torch.float32 and affine.shape == (B, 2) and affine.is_contiguous()
    if carry_out is None and carry_frames:
        carry_out = torch.empty((B, 3, O, H, W), dtype=torch.bfloat16, device=video.device)
    if carry_out is not None:
        assert tuple(carry_out.shape) == (B, 3, O, H, W) and carry_out.is_contiguous()
    shape = (B, max(write_hi - write_lo, 0), H, W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=video.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()
    _check(load_library().drn_postprocess_window_align_u8(_ptr(video), _ptr(prev_tail), _ptr(ramp_w), _ptr(affine), _ptr(out),
                                                          _ptr(carry_out), B, Tw, H, W, O, ramp_at, write_lo, write_hi,
                                                          1 if normalize_normal else 0, _stream()),
           "drn_postprocess_window_align_u8")
    return out, carry_out


def env_project(cube, vec, rot, log_scale=10000.0, out=None):
    """The forward renderer's environment light under a per-frame y-rotation (drn_env_project).  cube [6, R, R, 3], vec [H, W, 3]
    (latlong_vec), rot [T, 2] = (cos, sin) of every frame's angle, all fp32 and contiguous -> (env_ldr, env_log), each
    [3, T, H, W] fp32 in [-1, 1].  out: a pair of such tensors to write into."""
    for t in (cube, vec, rot):
        assert t.dtype == torch.float32 and t.is_contiguous(), "contiguous fp32 tensor required"
    R, (H, W), T = cube.shape[1], vec.shape[:2], rot.shape[0]
    assert cube.shape == (6, R, R, 3) and vec.shape == (H, W, 3) and rot.shape == (T, 2)
    if out is None:
        out = (torch.empty((3, T, H, W), dtype=torch.float32, device=cube.device),
               torch.empty((3, T, H, W), dtype=torch.float32, device=cube.device))
    for t in out:
        assert t.dtype == torch.float32 and t.shape == (3, T, H, W) and t.is_contiguous()
    _check(load_library().drn_env_project(_ptr(cube), R, _ptr(vec), _ptr(rot), _ptr(out[0]), _ptr(out[1]), T, H, W, log_scale,
                                          _stream()), "drn_env_project")
    return out


def env_cubes(latlong, grid, n0=0, n=None, brightness=1.0, flip=False, roll=0, out=None):
    """The cube maps of panoramas n0 .. n0 + n - 1 of an env-map sequence in one launch (drn_env_cubes).  latlong [N, He, We, 3]
    raw (preprocess_envmap.process_comfyui_sequence), grid [6, R, R, 2] (preprocess_envmap.cube_sample_grid), fp32 and
    contiguous; roll in [0, We) -> [n, 6, R, R, 3] fp32.  out: such a tensor to write into."""
    for t in (latlong, grid):
        assert t.dtype == torch.float32 and t.is_contiguous(), "contiguous fp32 tensor required"
    N, He, We = latlong.shape[:3]
    R = grid.shape[1]
    assert latlong.shape == (N, He, We, 3) and grid.shape == (6, R, R, 2)
    n = N - n0 if n is None else n
    if out is None:
        out = torch.empty((n, 6, R, R, 3), dtype=torch.float32, device=latlong.device)
    assert out.dtype == torch.float32 and out.shape == (n, 6, R, R, 3) and out.is_contiguous()
    _check(load_library().drn_env_cubes(_ptr(latlong), _ptr(grid), _ptr(out), N, He, We, R, n0, n, float(brightness),
                                        1 if flip else 0, int(roll), _stream()), "drn_env_cubes")
    return out


def env_project_seq(cubes, cube_of, vec, rot, log_scale=10000.0, out=None, t0=0):
    """drn_env_project with a cube map per frame (drn_env_project_seq).  cubes [n_cubes, 6, R, R, 3], vec [H, W, 3], rot [T, 2] on
    the device, fp32 and contiguous; cube_of int32 [T] on the HOST, every value checked to lie in [0, n_cubes) and then uploaded
    -> (env_ldr, env_log).  out: a pair of [3, T_all, H, W] tensors of which frames t0 .. t0 + T - 1 are written."""
    for t in (cubes, vec, rot):
        assert t.dtype == torch.float32 and t.is_contiguous(), "contiguous fp32 tensor required"
    n_cubes, R, (H, W), T = cubes.shape[0], cubes.shape[2], vec.shape[:2], rot.shape[0]
    assert cubes.shape == (n_cubes, 6, R, R, 3) and vec.shape == (H, W, 3) and rot.shape == (T, 2)
    assert not cube_of.is_cuda and cube_of.dtype == torch.int32 and cube_of.shape == (T,), "cube_of: int32 [T] on the host"
    assert 0 <= int(cube_of.min()) and int(cube_of.max()) < n_cubes, "cube_of outside the cube maps"
    if out is None:
        out = (torch.empty((3, T, H, W), dtype=torch.float32, device=cubes.device),
               torch.empty((3, T, H, W), dtype=torch.float32, device=cubes.device))
    T_all = out[0].shape[1]
    for t in out:
        assert t.dtype == torch.float32 and t.shape == (3, T_all, H, W) and t.is_contiguous()
    table = cube_of.contiguous().to(cubes.device)
    _check(load_library().drn_env_project_seq(_ptr(cubes), n_cubes, _ptr(table), R, _ptr(vec), _ptr(rot), _ptr(out[0]),
                                              _ptr(out[1]), T, t0, T_all, H, W, log_scale, _stream()), "drn_env_project_seq")
    return out


def _check_tap_table(lo_n, w, n_in):
    """One axis of a resampling plan as HOST tensors: lo_n int32 [n_out, 2], w fp32 [n_out, K <= 32], every row inside [0, n_in)."""
    assert lo_n.dtype == torch.int32 and w.dtype == torch.float32 and lo_n.ndim == 2 and w.ndim == 2
    assert lo_n.shape == (w.shape[0], 2) and 1 <= w.shape[1] <= 32, "tap table shapes"
    lo, n = lo_n[:, 0].long(), lo_n[:, 1].long()
    assert bool((lo >= 0).all()) and bool((n >= 1).all()) and bool((n <= w.shape[1]).all()) and bool((lo + n <= n_in).all()), \
        "taps outside the source"


def _fit_frames(symbol, dtype, what, src, t_idx, y_lo_n, y_w, x_lo_n, x_w, out):
    """drn_fit_frames / drn_fit_frames_u8: one argument list, the source's element type apart."""
    assert src.dtype == dtype and src.ndim == 5 and src.shape[-1] == 3 and src.is_contiguous(), \
        f"contiguous {what} [B, T, H, W, 3] frames required"
    B, Ts, Hs, Ws, _ = src.shape
    assert t_idx.dtype == torch.int32 and t_idx.ndim == 1 and 0 <= int(t_idx.min()) and int(t_idx.max()) < Ts, "t_idx outside the clip"
    _check_tap_table(y_lo_n, y_w, Hs)
    _check_tap_table(x_lo_n, x_w, Ws)
    Td, Hd, Wd = t_idx.shape[0], y_lo_n.shape[0], x_lo_n.shape[0]
    if out is None:
        out = torch.empty((B, 3, Td, Hd, Wd), dtype=torch.bfloat16, device=src.device)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (B, 3, Td, Hd, Wd) and out.is_contiguous()
    dev = [t.contiguous().to(src.device) for t in (t_idx, y_lo_n, y_w, x_lo_n, x_w)]
    _check(getattr(load_library(), symbol)(_ptr(src), _ptr(out), B, Ts, Hs, Ws, Td, Hd, Wd, _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]),
                                           y_w.shape[1], _ptr(dev[3]), _ptr(dev[4]), x_w.shape[1], _stream()), symbol)
    return out


def fit_frames(src, t_idx, y_lo_n, y_w, x_lo_n, x_w, out=None):
    """Clip ingest with a fit to the model's grid (drn_fit_frames; the plan: fit.plan_fit).  src [B, Ts, Hs, Ws, 3] fp32 on the
    device, contiguous; the plan's tables as HOST tensors (t_idx int32 [Td], per axis lo_n int32 [n_out, 2] and w fp32 [n_out, K]):
    they are checked here, where their contents can be read, and uploaded -> [B, 3, Td, Hd, Wd] bf16 in [-1, 1].  out: such a
    tensor to write into."""
    return _fit_frames("drn_fit_frames", torch.float32, "fp32", src, t_idx, y_lo_n, y_w, x_lo_n, x_w, out)


def fit_frames_u8(src, t_idx, y_lo_n, y_w, x_lo_n, x_w, out=None):
    """fit_frames from 8-bit frames (drn_fit_frames_u8): src [B, Ts, Hs, Ws, 3] uint8 on the device, contiguous, at any byte
    alignment; a byte i enters as fp32(i) / 255 correctly rounded, so the result is fit_frames on fit.u8_unit(src) bit for bit.
    The tables and `out` as for fit_frames."""
    return _fit_frames("drn_fit_frames_u8", torch.uint8, "uint8", src, t_idx, y_lo_n, y_w, x_lo_n, x_w, out)


def restore_frames(src, T, y_lo_n, y_w, x_lo_n, x_w, out=None):
    """The fit's way back on uint8 outputs (drn_restore_frames_u8; the plan: fit.plan_restore).  src [B, Ts, Hs, Ws, 3] uint8 on
    the device, contiguous, at any byte alignment; T <= Ts frames to return; the plan's tables as HOST tensors (per axis lo_n int32
    [n_out, 2] and w fp32 [n_out, K]): they are checked here, where their contents can be read, and uploaded -> uint8
    [B, T, Hd, Wd, 3].  out: such a tensor to write into."""
    assert src.dtype == torch.uint8 and src.ndim == 5 and src.shape[-1] == 3 and src.is_contiguous(), \
        "contiguous uint8 [B, T, H, W, 3] frames required"
    B, Ts, Hs, Ws, _ = src.shape
    assert 1 <= T <= Ts, "frames to return outside the clip"
    _check_tap_table(y_lo_n, y_w, Hs)
    _check_tap_table(x_lo_n, x_w, Ws)
    Hd, Wd = y_lo_n.shape[0], x_lo_n.shape[0]
    if out is None:
        out = torch.empty((B, T, Hd, Wd, 3), dtype=torch.uint8, device=src.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, T, Hd, Wd, 3) and out.is_contiguous()
    dev = [t.contiguous().to(src.device) for t in (y_lo_n, y_w, x_lo_n, x_w)]
    _check(load_library().drn_restore_frames_u8(_ptr(src), _ptr(out), B, Ts, Hs, Ws, T, Hd, Wd, _ptr(dev[0]), _ptr(dev[1]),
                                                y_w.shape[1], _ptr(dev[2]), _ptr(dev[3]), x_w.shape[1], _stream()),
           "drn_restore_frames_u8")
    return out


def restore_guided(src, guide_lo, guide_hi, T, y_lo_n, y_w, x_lo_n, x_w, range_tab, eps: float, t0: int = 0, out=None):
    """The guided way back on uint8 outputs (drn_restore_guided_u8; the plan: fit.plan_restore_guided).  src [B, Ts, Hs, Ws, 3],
    guide_lo [Bg, Tg, Hs, Ws, 3] and guide_hi [Bg, Tg, Hd, Wd, 3] uint8 on one device, contiguous, at any byte alignment, Bg 1 or B;
    T <= Ts frames to return, read from guide frames t0 .. t0 + T - 1; the plan's tables as HOST tensors (per axis lo_n int32
    [n_out, 2] and w fp32 [n_out, K <= 8], range_tab fp32 [256]): they are checked here, where their contents can be read, and
    uploaded -> uint8 [B, T, Hd, Wd, 3].  out: such a tensor to write into."""
    for t in (src, guide_lo, guide_hi):
        assert t.dtype == torch.uint8 and t.ndim == 5 and t.shape[-1] == 3 and t.is_contiguous() and t.device == src.device, \
            "contiguous uint8 [B, T, H, W, 3] frames on one device required"
    B, Ts, Hs, Ws, _ = src.shape
    Bg, Tg = guide_hi.shape[:2]
    Hd, Wd = y_lo_n.shape[0], x_lo_n.shape[0]
    assert Bg in (1, B), "one guide for every clip, or one per clip"
    assert tuple(guide_lo.shape) == (Bg, Tg, Hs, Ws, 3) and tuple(guide_hi.shape) == (Bg, Tg, Hd, Wd, 3), "guide shapes"
    assert 1 <= T <= Ts and 0 <= t0 and t0 + T <= Tg, "frames to return outside the clip or the guide"
    _check_tap_table(y_lo_n, y_w, Hs)
    _check_tap_table(x_lo_n, x_w, Ws)
    assert y_w.shape[1] <= 8 and x_w.shape[1] <= 8, "at most 8 taps per axis"
    assert range_tab.dtype == torch.float32 and tuple(range_tab.shape) == (256,) and eps > 0, "range table fp32 [256], eps > 0"
    if out is None:
        out = torch.empty((B, T, Hd, Wd, 3), dtype=torch.uint8, device=src.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, T, Hd, Wd, 3) and out.is_contiguous()
    dev = [t.contiguous().to(src.device) for t in (y_lo_n, y_w, x_lo_n, x_w, range_tab)]
    _check(load_library().drn_restore_guided_u8(_ptr(src), _ptr(guide_lo), _ptr(guide_hi), _ptr(out), B, Bg, Ts, Hs, Ws, Tg, t0, T,
                                                Hd, Wd, _ptr(dev[0]), _ptr(dev[1]), y_w.shape[1], _ptr(dev[2]), _ptr(dev[3]),
                                                x_w.shape[1], _ptr(dev[4]), float(eps), _stream()), "drn_restore_guided_u8")
    return out


def tile_blend_u8(canvas, tile, wy, wx, y_at: int, x_at: int, ry: int, rx: int):
    """One spatial tile into the picture's canvas, in place (drn_tile_blend_u8; the plan: tiles.plan_tiles).  canvas [B,T,H,W,3]
    and tile [B,T,h,w,3] uint8 on the device, contiguous, at any byte alignment; the tile's rows from ry and columns from rx on
    land at (y_at + ry, x_at + rx), the first len(wy) written rows and len(wx) written columns cross-faded over what the canvas
    holds.  wy / wx: fp32 ramp weights on the device, or None for no ramp on that axis.  Returns the canvas."""
    for t in (canvas, tile):
        assert t.dtype == torch.uint8 and t.ndim == 5 and t.shape[-1] == 3 and t.is_contiguous(), \
            "contiguous uint8 [B, T, H, W, 3] frames required"
    B, T, H, W, _ = canvas.shape
    h, w = tile.shape[2:4]
    assert tuple(tile.shape[:2]) == (B, T) and tile.device == canvas.device, "canvas and tile are one clip on one device"
    O = []
    for name, t in (("wy", wy), ("wx", wx)):
        if t is not None:
            assert t.dtype == torch.float32 and t.ndim == 1 and t.numel() > 0 and t.is_contiguous() and t.device == canvas.device, \
                f"{name}: a non-empty contiguous fp32 vector on the canvas's device, or None"
        O.append(0 if t is None else t.numel())
    _check(load_library().drn_tile_blend_u8(_ptr(canvas), _ptr(tile), _ptr(wy), _ptr(wx), B * T, H, W, h, w, y_at, x_at, ry, rx,
                                            O[0], O[1], _stream()), "drn_tile_blend_u8")
    return canvas


ENSEMBLE_MODES = {"median": 0, "mean": 1, "normal": 2}


def ensemble_reduce_u8(members, mode: str, spread: bool = False):
    """N uint8 results of one shape reduced per pixel in one launch (drn_ensemble_reduce_u8; the specification:
    ensemble.reduce_members).  members: 1..16 uint8 tensors of one shape [..., 3] on one device, each contiguous (they need not
    lie in one allocation: their pointers go to the kernel by value, no stack is built); mode: 'median' / 'mean' / 'normal'.
    -> (the result, the spread or None), both of the members' shape."""
    N = len(members)
    first = members[0]
    for m in members:
        assert m.dtype == torch.uint8 and m.is_contiguous() and m.shape == first.shape and m.device == first.device, \
            "contiguous uint8 tensors of one shape on one device required"
    assert first.ndim >= 1 and first.shape[-1] == 3, "[..., 3] pixels required"
    out = torch.empty_like(first)
    sp = torch.empty_like(first) if spread else None
    table = (c_void_p * N)(*[_ptr(m) for m in members])
    _check(load_library().drn_ensemble_reduce_u8(table, N, _ptr(out), _ptr(sp), first.numel(), ENSEMBLE_MODES[mode], _stream()),
           "drn_ensemble_reduce_u8")
    return out, sp


def _ensemble_clips(members):
    """The checks the two aligned entries share -> (N, B, clip_bytes): contiguous uint8 [B, ..., 3] tensors of one shape."""
    first = members[0]
    for m in members:
        assert m.dtype == torch.uint8 and m.is_contiguous() and m.shape == first.shape and m.device == first.device, \
            "contiguous uint8 tensors of one shape on one device required"
    assert first.ndim >= 2 and first.shape[-1] == 3 and first.shape[0] >= 1, "[B, ..., 3] pixels required"
    return len(members), int(first.shape[0]), first.numel() // int(first.shape[0])


def ensemble_align_affine(members, stats: bool = False):
    """One gain and offset per member and clip, from the members' Gram matrix over the whole clip, solved on the device in two
    launches (drn_ensemble_align_affine; the specification: ensemble.align_members).  members: 1..16 contiguous uint8 tensors
    [B, ..., 3] of one shape on one device, clip b = member[b] -> affine [N, B, 2] fp32 = (g, o) on the device, never read by the
    host; with stats=True also the fp64 [B, N + N * N] means and covariances behind it."""
    N, B, clip_bytes = _ensemble_clips(members)
    first = members[0]
    lib = load_library()
    nbytes = lib.drn_ensemble_align_workspace_bytes(N, B, clip_bytes)
    ws = torch.empty(max(nbytes, 8) // 8 + 1, dtype=torch.int64, device=first.device)
    affine = torch.empty((N, B, 2), dtype=torch.float32, device=first.device)
    st = torch.empty((B, N + N * N), dtype=torch.float64, device=first.device) if stats else None
    table = (c_void_p * N)(*[_ptr(m) for m in members])
    _check(lib.drn_ensemble_align_affine(table, N, B, clip_bytes, _ptr(affine), _ptr(st), _ptr(ws), ws.numel() * 8, _stream()),
           "drn_ensemble_align_affine")
    return (affine, st) if stats else affine


def ensemble_reduce_affine_u8(members, affine, mode: str, spread: bool = False):
    """ensemble_reduce_u8 in the modes 'median' / 'mean' with every member's byte read through its clip's affine
    (drn_ensemble_reduce_affine_u8; the specification: ensemble.reduce_members with an affine).  members: as in
    ensemble_align_affine; affine: fp32 [N, B, 2] on their device, finite.  -> (the result, the spread or None)."""
    N, B, clip_bytes = _ensemble_clips(members)
    first = members[0]
    assert mode in ("median", "mean"), "normal maps are never aligned"
    assert affine.dtype == torch.float32 and tuple(affine.shape) == (N, B, 2) and affine.is_contiguous() and \
        affine.device == first.device, "affine: contiguous fp32 [N, B, 2] on the members' device"
    out = torch.empty_like(first)
    sp = torch.empty_like(first) if spread else None
    table = (c_void_p * N)(*[_ptr(m) for m in members])
    _check(load_library().drn_ensemble_reduce_affine_u8(table, N, _ptr(affine), B, clip_bytes, _ptr(out), _ptr(sp),
                                                        ENSEMBLE_MODES[mode], _stream()), "drn_ensemble_reduce_affine_u8")
    return out, sp


def _frame_strides(name, t, B, T, frame_shape):
    """A uint8 tensor [1 or B, 1 or T, *frame_shape] whose frames are contiguous -> (batch stride, frame stride) in bytes, 0 where
    the axis is broadcast."""
    assert t.dtype == torch.uint8 and t.ndim == 2 + len(frame_shape) and tuple(t.shape[2:]) == tuple(frame_shape), \
        f"{name}: uint8 [B, T, {', '.join(str(n) for n in frame_shape)}] required, got {t.dtype} {tuple(t.shape)}"
    assert t.shape[0] in (1, B) and t.shape[1] in (1, T), f"{name}: {tuple(t.shape[:2])} clips and frames for {(B, T)}"
    assert t[0, 0].is_contiguous() and t.stride(0) >= 0 and t.stride(1) >= 0, f"{name}: contiguous frames required"
    return (t.stride(0) if t.shape[0] > 1 else 0), (t.stride(1) if t.shape[1] > 1 else 0)


def gbuffer_edit_u8(maps, edit_mask=None, insert_mask=None):
    """Material edits and layer insertion on 1..5 G-buffers in one launch (drn_gbuffer_edit_u8; the rule and the specification:
    gbuffer_edit.edit_gbuffers).  maps: a list of (src, dst, layer or None, gain[3], offset[3], is_normal); src and dst uint8
    [B, T, H, W, 3] on one device with contiguous frames - a batch-strided [:, :keep] view is fine -, dst the same tensor as src
    (in place) or one that overlaps nothing; layer uint8 [1 or B, 1 or T, H, W, 3].  edit_mask, insert_mask: uint8
    [1 or B, 1 or T, H, W] or None.  Returns the dsts."""
    first = maps[0][0]
    B, T, H, W, _ = first.shape
    table = (GbufferEditMap * len(maps))()
    for k, (src, dst, layer, gain, offset, is_normal) in enumerate(maps):
        e = table[k]
        assert src.device == first.device and dst.device == first.device and tuple(src.shape) == tuple(dst.shape) == (B, T, H, W, 3), \
            "the maps of a call are uint8 [B, T, H, W, 3] tensors of one shape on one device"
        e.src, e.dst = _ptr(src), _ptr(dst)
        e.src_bs, e.src_ts = _frame_strides("src", src, B, T, (H, W, 3))
        e.dst_bs, e.dst_ts = _frame_strides("dst", dst, B, T, (H, W, 3))
        if layer is not None:
            assert layer.device == first.device, "a layer lives on the maps' device"
            e.layer = _ptr(layer)
            e.layer_bs, e.layer_ts = _frame_strides("layer", layer, B, T, (H, W, 3))
        for c in range(3):
            e.gain[c], e.offset[c] = float(gain[c]), float(offset[c])
        e.is_normal = int(bool(is_normal))
    ms = []
    for name, m in (("edit_mask", edit_mask), ("insert_mask", insert_mask)):
        if m is not None:
            assert m.device == first.device, f"{name} lives on the maps' device"
        ms.append((0, 0) if m is None else _frame_strides(name, m, B, T, (H, W)))
    _check(load_library().drn_gbuffer_edit_u8(table, len(maps), _ptr(edit_mask), ms[0][0], ms[0][1], _ptr(insert_mask), ms[1][0],
                                              ms[1][1], B, T, H * W, _stream()), "drn_gbuffer_edit_u8")
    return [m[1] for m in maps]


def _latent_canvas(name, t):
    _bf16(t)
    assert t.ndim >= 3 and t.is_contiguous(), f"{name}: a contiguous bf16 [..., H, W] tensor required"
    return t.numel() // (t.shape[-2] * t.shape[-1]), t.shape[-2], t.shape[-1]


def latent_tile_gather(canvas, h: int, w: int, y_at: int, x_at: int, c_in: float, copies: int = 1):
    """One tile's crop of the latent canvas as the DiT's input (drn_latent_tile_gather; the plan: tiles.latent_tile).  canvas
    [P, C, F, Hc, Wc] bf16 on the device, contiguous -> [copies * P, C, F, h, w] bf16 = edm_scale_input of the crop at
    (y_at, x_at), `copies` (1, or 2 under CFG) times along the batch."""
    planes, Hc, Wc = _latent_canvas("canvas", canvas)
    out = torch.empty((copies * canvas.shape[0], *canvas.shape[1:-2], h, w), dtype=torch.bfloat16, device=canvas.device)
    _check(load_library().drn_latent_tile_gather(_ptr(canvas), _ptr(out), planes, Hc, Wc, h, w, y_at, x_at, c_in, copies, _stream()),
           "drn_latent_tile_gather")
    return out


def latent_tile_step_join(model_out, uncond, guidance: float, canvas_cur, canvas_next, wy, wx, y_at: int, x_at: int, ry: int,
                          rx: int, c_skip: float, c_out: float, sigma: float, dt: float):
    """CFG combine, Euler step and cross-fade of one tile's DiT output into the next latent canvas, in place
    (drn_latent_tile_step_join; the specification: tiles.latent_step_join).  model_out (and uncond, or None for no CFG)
    [P, C, F, h, w], canvas_cur and canvas_next [P, C, F, Hc, Wc], all bf16 on one device, contiguous; the tile's rows from ry and
    columns from rx on land at (y_at + ry, x_at + rx), the first len(wy) written rows and len(wx) written columns cross-faded over
    what canvas_next holds.  wy / wx: fp32 ramp weights on the device, or None for no ramp on that axis.  Returns canvas_next."""
    planes, Hc, Wc = _latent_canvas("canvas_cur", canvas_cur)
    assert _latent_canvas("canvas_next", canvas_next) == (planes, Hc, Wc), "the two canvases have one shape"
    tp, h, w = _latent_canvas("model_out", model_out)
    assert tp == planes, "tile and canvas have the same planes"
    if uncond is not None:
        assert _latent_canvas("uncond", uncond) == (planes, h, w), "uncond has the tile's shape"
    O = []
    for name, t in (("wy", wy), ("wx", wx)):
        if t is not None:
            assert t.dtype == torch.float32 and t.ndim == 1 and t.numel() > 0 and t.is_contiguous() and t.device == canvas_cur.device, \
                f"{name}: a non-empty contiguous fp32 vector on the canvas's device, or None"
        O.append(0 if t is None else t.numel())
    _check(load_library().drn_latent_tile_step_join(_ptr(model_out), _ptr(uncond), guidance, _ptr(canvas_cur), _ptr(canvas_next),
                                                    _ptr(wy), _ptr(wx), planes, Hc, Wc, h, w, y_at, x_at, ry, rx, O[0], O[1], c_skip,
                                                    c_out, sigma, dt, _stream()), "drn_latent_tile_step_join")
    return canvas_next


def _stamp(args: "DitForwardArgs"):
    """The two fields of the argument block the binding owns: its size (the ABI check) and the timer handle."""
    args.struct_bytes = ctypes.sizeof(DitForwardArgs)
    if _TIMER is not None:
        h = _TIMER.native_handle()
        args.timer = h.value if h is not None else None
    else:
        args.timer = None


def dit_forward(args: "DitForwardArgs"):
    """Enqueue one whole DiT forward (drn_dit_forward).  `args` holds raw pointers: the caller keeps every tensor alive."""
    _stamp(args)
    _check(load_library().drn_dit_forward(ctypes.byref(args), _stream()), "drn_dit_forward")


DIT_EMBED, DIT_FINAL = 1, 2


def dit_forward_range(args: "DitForwardArgs", sub_lo: int, sub_hi: int, flags: int):
    """Enqueue a part of a DiT forward (drn_dit_forward_range): the patch embed (DIT_EMBED), the sub-blocks [sub_lo, sub_hi), the
    final layer (DIT_FINAL).  `args` as for dit_forward; parts that tile the forward give its bits."""
    _stamp(args)
    _check(load_library().drn_dit_forward_range(ctypes.byref(args), int(sub_lo), int(sub_hi), int(flags), _stream()),
           "drn_dit_forward_range")


def _clips(t):
    _bf16(t)
    assert t.is_contiguous() and t.ndim >= 2 and t.numel() > 0
    return t.shape[0], t.numel() // t.shape[0]


def step_cache_probe(x, ref, stats=None, workspace=None):
    """How far `x` [B, ...] bf16 lies from `ref` of the same shape, per clip of the leading dimension (drn_step_cache_probe; the
    specification: step_cache.probe_reference) -> stats [B, 2] fp64 = (sum |x - ref|, sum |ref|) on the device, never read here."""
    B, n = _clips(x)
    assert _clips(ref) == (B, n)
    lib = load_library()
    nbytes = lib.drn_step_cache_workspace_bytes(B, n)
    if workspace is None:
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    assert workspace.dtype == torch.float64 and workspace.numel() * 8 >= nbytes
    if stats is None:
        stats = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (B, 2) and stats.is_contiguous()
    _check(lib.drn_step_cache_probe(_ptr(x), _ptr(ref), _ptr(stats), _ptr(workspace), workspace.numel() * 8, B, n, _stream()),
           "drn_step_cache_probe")
    return stats


def step_cache_residual(x, ref, out=None):
    """bf16(fp32(x) - fp32(ref)) (drn_step_cache_residual), into `out` or a new tensor."""
    _bf16(x, ref, out)
    if out is None:
        out = torch.empty_like(x)
    assert x.is_contiguous() and ref.is_contiguous() and out.is_contiguous() and x.numel() == ref.numel() == out.numel()
    _check(load_library().drn_step_cache_residual(_ptr(x), _ptr(ref), _ptr(out), x.numel(), _stream()), "drn_step_cache_residual")
    return out


def step_cache_apply(x, r):
    """x <- bf16(fp32(x) + fp32(r)) in place (drn_step_cache_apply)."""
    _bf16(x, r)
    assert x.is_contiguous() and r.is_contiguous() and x.numel() == r.numel()
    _check(load_library().drn_step_cache_apply(_ptr(x), _ptr(r), x.numel(), _stream()), "drn_step_cache_apply")
    return x
