"""ctypes binding of libdcv_hip.so (include/dcv.h).  Thin: tensors in, raw device pointers +
sizes + the current torch stream out.  There is NO fallback: if the library is missing or a call
returns an error code, this raises.  PyTorch is used only for device memory and streams."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCV_LIB", os.path.join(_HERE, "libdcv_hip.so"))  # DCV_LIB: A/B builds of the same ABI

EPI_BIAS_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_PLAIN_BF16, EPI_GELU_BWD_BF16, EPI_PATCH = range(6)
TILE_AUTO, TILE_NARROW, TILE_WIDE, TILE_PAIR, TILE_ALT, TILE_WS, TILE_AUTO_WS = range(7)  # include/dcv.h DCV_TILE_* (TILE_ALT is retired: refused)

_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
_SIGS = {
    "dcv_version": ([], C.c_int),
    "dcv_error_string": ([_i], C.c_char_p),
    "dcv_gemm_nt": ([_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp], _i),
    "dcv_gemm_nt_ex": ([_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp], _i),
    "dcv_gemm_nt_pick": ([_i, _i, _i, _i, _i], _i),
    "dcv_gemm_nt384_plan": ([_i, _i, _i, _vp, _vp], _i),
    "dcv_gemm_nt_resid_ln": ([_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _f, _vp, _i, _vp, _vp, _i, _vp], _i),
    "dcv_gemm_tn_pick": ([_i, _i, _i, _i], _i),
    "dcv_gemm_tn_acc": ([_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp], _i),
    "dcv_gemm_tn_acc_ex": ([_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp], _i),
    "dcv_gemm_tn_det_ws_floats": ([_i, _i, _i, _i], _l),
    "dcv_gemm_tn_acc_det": ([_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _l, _vp], _i),
    "dcv_gemm_tn_group_ws_floats": ([_vp, _i, _i], _l),
    "dcv_gemm_tn_group": ([_vp, _i, _i, _vp, _l, _vp], _i),
    "dcv_bias_grad_ws_floats": ([_i, _i], _l),
    "dcv_bias_grad": ([_vp, _i, _i, _i, _vp, _vp, _l, _vp], _i),
    "dcv_bias_grad_plan": ([_i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "dcv_ln_fwd": ([_vp, _l, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _vp], _i),
    "dcv_ln_pool_channels_ws_floats": ([_i, _i, _i, _i], _l),
    "dcv_ln_pool_channels": ([_vp, _vp, _vp, _f, _vp, _i, _i, _i, _i, _vp, _l, _vp], _i),
    "dcv_ln_pool_channels_bwd_ws_floats": ([_i, _i, _i, _i], _l),
    "dcv_ln_pool_channels_bwd": ([_vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _l, _vp], _i),
    "dcv_ln_bwd": ([_vp, _i, _vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _i, _i, _vp], _i),
    "dcv_ln_bwd_det_ws_floats": ([_i, _i], _l),
    "dcv_ln_bwd_det": ([_vp, _i, _vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _i, _i, _vp, _l, _vp], _i),
    "dcv_ln_bwd_scaled": ([_vp, _i, _vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _l, _vp], _i),
    "dcv_patch_bwd_det_ws_floats": ([_i, _i, _i, _i], _l),
    "dcv_patch_bwd_det": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _l, _vp], _i),
    "dcv_ortho_fwd_det_ws_floats": ([_i, _i, _i, _i], _l),
    "dcv_ortho_fwd_det": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _l, _vp], _i),
    "dcv_sumsq_det_ws_floats": ([_l], _l),
    "dcv_sumsq_acc_det": ([_vp, _l, _vp, _vp, _l, _vp], _i),
    "dcv_attn_fwd": ([_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd_delta": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "dcv_attn_bwd_dq": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd_dkdv": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_fwd_rows": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd_rows": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd_dq_rows": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd_dkdv_rows": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_fwd_rows_ps": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "dcv_attn_bwd_rows_ps": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd_dq_rows_ps": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_bwd_dkdv_rows_ps": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_probs_rows": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_probs_rows_ps": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "dcv_attn_channel_mass_ws_floats": ([_i, _i, _i, _i], _l),
    "dcv_attn_channel_mass": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _i, _vp, _l, _vp], _i),
    "dcv_attn_channel_mass_ps": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _l, _vp], _i),
    "dcv_attn_rollout_step": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp], _i),
    "dcv_attn_rollout_step_ps": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_relevance_step": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "dcv_attn_relevance_step_ps": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "dcv_im2col_bf16": ([_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "dcv_patch_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "dcv_patch_dgrad": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "dcv_gather_tokens": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "dcv_fill_cls": ([_vp, _vp, _vp, _i, _l, _i, _vp], _i),
    "dcv_tps_warp": ([_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "dcv_crop_resize_flip": ([_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "dcv_ortho_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "dcv_ortho_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "dcv_proxy_loss_supported": ([_i, _i], _i),
    "dcv_proxy_loss": ([_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp], _i),
    "dcv_dino_loss_ws_floats": ([_i, _i, _i], _l),
    "dcv_dino_loss_fwd": ([_vp, _l, _vp, _l, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _l, _vp], _i),
    "dcv_dino_loss_bwd": ([_vp, _l, _vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _l, _vp], _i),
    "dcv_dino_loss_plan": ([_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "dcv_ibot_loss_ws_floats": ([_i, _i], _l),
    "dcv_ibot_loss_fwd": ([_vp, _l, _vp, _l, _vp, _vp, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _l, _vp], _i),
    "dcv_ibot_loss_bwd": ([_vp, _l, _vp, _l, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _vp, _l, _vp], _i),
    "dcv_ibot_loss_plan": ([_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "dcv_mask_tokens_fwd": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "dcv_mask_tokens_bwd_ws_floats": ([_i, _i, _i, _i], _l),
    "dcv_mask_tokens_bwd": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _l, _vp], _i),
    "dcv_adamw": ([_vp, _vp, _vp, _vp, _l, _f, _f, _f, _f, _f, _i, _f, _vp], _i),
    "dcv_adamw_dyn": ([_vp, _vp, _vp, _vp, _l, _vp, _vp], _i),
    "dcv_adamw_set_hyper": ([_vp, _f, _f, _f, _f, _f, _i, _f, _vp], _i),
    "dcv_adamw_set_hyper_groups": ([_vp, _vp, _vp, _i, _f, _vp], _i),
    "dcv_adamw_groups": ([_vp, _vp, _vp, _vp, _l, _vp, _vp, _i, _vp, _i, _vp], _i),
    "dcv_avg_update": ([_vp, _vp, _l, _i, _f, _l, _vp, _i, _vp], _i),
    "dcv_cast_bf16": ([_vp, _vp, _l, _vp], _i),
    "dcv_cast_transpose_bf16": ([_vp, _vp, _vp, _i, _i, _vp], _i),
    "dcv_sumsq_acc": ([_vp, _l, _vp, _vp], _i),
    "dcv_clip_scale": ([_vp, _l, _vp, _f, _vp], _i),
    "dcv_cast_bf16_sr": ([_vp, _vp, _l, _vp, _vp], _i),
    "dcv_cast_transpose_bf16_sr": ([_vp, _vp, _vp, _i, _i, _vp, _vp], _i),
    "dcv_cast_scaled_ranges": ([_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp], _i),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load() -> C.CDLL:
    """Loads the in-tree library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is the only compute path of diverse_channel_vit_amd. "
                "Build it with `python -m diverse_channel_vit_amd._build` (needs hipcc, gfx950).")
        lib = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
        _lib = lib
    return _lib


# optional per-kernel timing with events on the launch stream (bench.py).  Records are keyed by the device SYMBOL the entry
# launches plus its problem shape, e.g. ("gemm_nt384_kernel<1>", "M100416 N1536 K384"); every record carries the algorithmic
# and the executed FLOPs and the algorithmic HBM bytes of that launch.
_prof = None          # None | {key: {"ev": [(start, end)], "flops": f, "flops_exec": f, "bytes": b}}
_prof_only = None     # None | set of symbols to time (everything when None)


def set_profiler(enable=False, only=None):
    """enable: start a fresh record set (False/None disables).  only: iterable of symbols to time.  Returns the previous records."""
    global _prof, _prof_only
    old = _prof
    _prof = {} if enable else None
    _prof_only = None if only is None else set(only)
    return old


class _timed:
    def __init__(self, symbol, shape="", flops=0.0, flops_exec=None, nbytes=0.0):
        self.rec = None
        if _prof is not None and (_prof_only is None or symbol in _prof_only):
            self.rec = _prof.setdefault((symbol, shape), {"ev": [], "flops": float(flops), "flops_exec": float(flops if flops_exec is None else flops_exec),
                                                          "bytes": float(nbytes)})

    def __enter__(self):
        if self.rec is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *a):
        if self.rec is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.rec["ev"].append((self.s, e))


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULL = _Null()


def _timer(describe):
    """describe() -> (symbol, shape, flops, flops_exec, bytes); evaluated only while profiling (no host cost otherwise)."""
    if _prof is None:
        return _NULL
    return _timed(*describe())


_EPI_OUT_BYTES = {0: 2, 1: 4, 2: 4, 3: 2, 4: 2, 5: 8}   # bytes written per output element (GELU: two bf16; PATCH: tokens + pre-embedding copy)
_EPI_AUX_BYTES = {0: 0, 1: 0, 2: 4, 3: 0, 4: 2, 5: 0}   # bytes read per output element besides the operands (residual f32, saved GELU' bf16)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: {load().dcv_error_string(rc).decode()} ({rc})")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")


# ---------------------------------------------------------------------------------------------
# Deterministic mode — the DEFAULT since round 3 (the reference's trainer sets cudnn.deterministic = True, utils.py:394-401).  Every entry
# that would add partial sums of several workgroups with atomics runs in its *_det form: partials through a workspace, summed in a
# fixed order by a second launch — a training step is bit-reproducible.  Cost measured on the headline step: 35.52 -> 35.78 ms (+0.7 %; the
# weight-gradient GEMMs are 5-7 % FASTER with plain partial stores + one reduction pass than with their fp32-atomic flush, LayerNorm's
# 23 extra reduction launches cost the rest).  set_deterministic(False) / DCV_DETERMINISTIC=0 selects the atomic forms.  One workspace per
# (device, stream), grown on demand; kernels on one stream run in order, so they can share it.
_deterministic = os.environ.get("DCV_DETERMINISTIC", "1") not in ("0", "", "false", "False")
_det_ws = {}
_det_ws_retired = []  # outgrown workspaces, kept alive (see _workspace)


def set_deterministic(on: bool = True) -> bool:
    """Returns the previous setting."""
    global _deterministic
    old, _deterministic = _deterministic, bool(on)
    return old


def is_deterministic() -> bool:
    return _deterministic


def _workspace(n_floats: int, like: torch.Tensor) -> torch.Tensor:
    key = (like.device.index, torch.cuda.current_stream(like.device).cuda_stream)
    ws = _det_ws.get(key)
    if ws is None or ws.numel() < n_floats:
        if ws is not None:
            # never freed: a captured HIP graph (graph.GraphedTrainStep) replays launches that carry the OLD workspace's address; handing
            # that block back to the allocator would let replays write partial tiles into somebody else's memory.  Growth is
            # rare (the first steps of a run) and the sizes small (<= 50 MB each).
            _det_ws_retired.append(ws)
        ws = torch.empty(max(int(n_floats), 1 << 20), dtype=torch.float32, device=like.device)
        _det_ws[key] = ws
    return ws


def _ws_size(n) -> int:
    if n < 0:
        _check(int(n), "det workspace size")
    return int(n)


def gemm_nt(A, W, epilogue, out, *, bias=None, out2=None, aux=None, aux2=None, T=0, n=0, ldo=None, ldo2=None, ldaux=None,
            grid_cap=0, tile=TILE_AUTO_WS):
    """C = A[M,K] @ W[N,K]^T with the given epilogue (see include/dcv.h).  grid_cap / tile: dcv_gemm_nt_ex's launch controls."""
    _req(A, torch.bfloat16, "A"); _req(W, torch.bfloat16, "W")
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K
    ldo = out.shape[-1] if ldo is None else ldo
    ldo2 = (out2.shape[-1] if out2 is not None else 0) if ldo2 is None else ldo2
    ldaux = (aux.shape[-1] if aux is not None else 0) if ldaux is None else ldaux
    lib = load()

    def describe():
        kind = {TILE_WIDE: "gemm_nt384", TILE_PAIR: "gemm_nt_pair", TILE_WS: "gemm_nt_ws"}.get(lib.dcv_gemm_nt_pick(M, N, K, epilogue, tile), "gemm_nt")
        nbytes = 2.0 * M * K + 2.0 * N * K + M * N * (_EPI_OUT_BYTES[epilogue] + _EPI_AUX_BYTES[epilogue])
        return f"{kind}_kernel<{epilogue}>", f"M{M} N{N} K{K}", 2.0 * M * N * K, None, nbytes

    with _timer(describe):
        rc = lib.dcv_gemm_nt_ex(_p(A), K, _p(W), K, M, N, K, epilogue, _p(bias), _p(out), ldo, _p(out2), ldo2, _p(aux), ldaux,
                                   _p(aux2), T, n, grid_cap, tile, _stream())
    _check(rc, "dcv_gemm_nt")


def gemm_nt_resid_ln(A, W, bias, resid, x_out, gamma, beta, eps, u_out, mean, rstd, *, branch_scale=None, T=0, grid_cap=0):
    """x_out = resid + s (A W^T + bias) and u_out = LayerNorm(x_out) * gamma + beta (bf16), mean / rstd per row, in ONE launch of the
    256 x 384 kernel (include/dcv.h: dcv_gemm_nt_resid_ln; N must be 384).  x_out may alias resid."""
    _req(A, torch.bfloat16, "A"); _req(W, torch.bfloat16, "W"); _req(u_out, torch.bfloat16, "u_out")
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K and x_out.shape[-1] == N and u_out.shape[-1] == N and resid.shape[-1] == N
    lib = load()
    # the residual GEMM's bytes plus the bf16 LayerNorm output and the row statistics; FLOPs of the product
    nbytes = 2.0 * M * K + 2.0 * N * K + M * N * (4 + 4 + 2) + 8.0 * M
    with _timer(lambda: ("gemm_nt384_kernel<6>", f"M{M} N{N} K{K}", 2.0 * M * N * K, None, nbytes)):
        rc = lib.dcv_gemm_nt_resid_ln(_p(A), K, _p(W), K, M, N, K, _p(bias), _p(resid), N, _p(branch_scale), T, _p(x_out), N, _p(gamma), _p(beta),
                                      float(eps), _p(u_out), N, _p(mean), _p(rstd), grid_cap, _stream())
    _check(rc, "dcv_gemm_nt_resid_ln")


def gemm_tn_det_ws_floats(M, P, Q, tile=TILE_AUTO) -> int:
    n = load().dcv_gemm_tn_det_ws_floats(M, P, Q, tile)
    if n < 0:
        _check(int(n), "dcv_gemm_tn_det_ws_floats")
    return int(n)


class _TnItem(C.Structure):  # include/dcv.h: dcv_tn_item
    _fields_ = [("Y", C.c_void_p), ("X", C.c_void_p), ("dW", C.c_void_p), ("dbias", C.c_void_p),
                ("ldy", C.c_int), ("ldx", C.c_int), ("P", C.c_int), ("Q", C.c_int), ("lddw", C.c_int), ("reserved", C.c_int)]


def gemm_tn_group_supported(shapes, M) -> bool:
    """shapes: iterable of (P, Q).  True when dcv_gemm_tn_group takes them in one launch on this device (every P % 384 == 0, Q % 128 == 0,
    all tiles in one resident round)."""
    shapes = list(shapes)
    if not 1 <= len(shapes) <= 8:
        return False
    arr = (_TnItem * len(shapes))()
    for it, (P, Q) in zip(arr, shapes):
        it.Y = it.X = it.dW = 16  # non-null, aligned placeholders: the size query reads shapes only
        it.ldy, it.ldx, it.P, it.Q, it.lddw = P, Q, P, Q, Q
    return load().dcv_gemm_tn_group_ws_floats(C.cast(arr, C.c_void_p), len(shapes), M) >= 0


def gemm_tn_acc_group(items):
    """items: list of (Y [M,P] bf16, X [M,Q] bf16, dW [P,Q] f32, dbias [P] f32 or None) over the SAME M rows: every dW += Y^T X and dbias +=
    colsum(Y) in ONE launch (dcv_gemm_tn_group); deterministic mode takes the partial tiles through the per-stream workspace."""
    lib = load()
    n = len(items)
    arr = (_TnItem * n)()
    M = items[0][0].shape[0]
    flops = 0.0
    nbytes = 0.0
    for it, (Y, X, dW, db) in zip(arr, items):
        _req(Y, torch.bfloat16, "Y"); _req(X, torch.bfloat16, "X"); _req(dW, torch.float32, "dW")
        if Y.shape[0] != M or X.shape[0] != M or dW.shape != (Y.shape[1], X.shape[1]):
            raise ValueError("gemm_tn_acc_group: every item is (Y [M,P], X [M,Q], dW [P,Q]) over the same M")
        it.Y, it.X, it.dW, it.dbias = Y.data_ptr(), X.data_ptr(), dW.data_ptr(), (db.data_ptr() if db is not None else None)
        it.ldy, it.ldx, it.P, it.Q, it.lddw = Y.stride(0), X.stride(0), Y.shape[1], X.shape[1], dW.stride(0)
        flops += 2.0 * M * Y.shape[1] * X.shape[1]
        nbytes += 2.0 * M * (Y.shape[1] + X.shape[1]) + 8.0 * Y.shape[1] * X.shape[1]
    ptr = C.cast(arr, C.c_void_p)
    ws = None
    if _deterministic:
        ws = _workspace(_ws_size(lib.dcv_gemm_tn_group_ws_floats(ptr, n, M)), items[0][2])
    shape = f"M{M} " + "+".join(f"{it.P}x{it.Q}" for it in arr)
    with _timer(lambda: ("gemm_tn384_group_kernel", shape, flops, flops, nbytes)):
        rc = lib.dcv_gemm_tn_group(ptr, n, M, _p(ws), ws.numel() if ws is not None else 0, _stream())
    _check(rc, "dcv_gemm_tn_group")


def gemm_tn_acc(Y, X, dW, dbias=None, tile=TILE_AUTO, ws=None):
    """dW[P,Q] += Y[M,P]^T @ X[M,Q]; dbias[P] += colsum(Y).  ws (fp32 scratch of >= gemm_tn_det_ws_floats elements): the deterministic
    form — partial tiles through ws, summed in a fixed order (dcv_gemm_tn_acc_det) — instead of fp32 atomics."""
    _req(Y, torch.bfloat16, "Y"); _req(X, torch.bfloat16, "X"); _req(dW, torch.float32, "dW")
    M, P = Y.shape
    Q = X.shape[1]
    assert X.shape[0] == M and dW.numel() == P * Q
    lib = load()
    if ws is None and _deterministic:
        ws = _workspace(_ws_size(lib.dcv_gemm_tn_det_ws_floats(M, P, Q, tile)), dW)
    with _timer(lambda: ("gemm_tn384_kernel" if lib.dcv_gemm_tn_pick(M, P, Q, tile) == TILE_WIDE else "gemm_tn_kernel", f"M{M} P{P} Q{Q}",
                         2.0 * M * P * Q, None, 2.0 * M * (P + Q) + 8.0 * P * Q)):
        if ws is None:
            rc = lib.dcv_gemm_tn_acc_ex(_p(Y), P, _p(X), Q, M, P, Q, _p(dW), Q, _p(dbias), tile, _stream())
        else:
            _req(ws, torch.float32, "ws")
            rc = lib.dcv_gemm_tn_acc_det(_p(Y), P, _p(X), Q, M, P, Q, _p(dW), Q, _p(dbias), tile, _p(ws), ws.numel(), _stream())
    _check(rc, "dcv_gemm_tn_acc")


def bias_grad_ws_floats(M, P) -> int:
    return _ws_size(load().dcv_bias_grad_ws_floats(M, P))


def bias_grad(Y, dbias, ws=None):
    """dbias[P] += colsum(Y[M,P]) — gemm_tn_acc's bias gradient without the product (include/dcv.h: dcv_bias_grad), for a Linear whose bias
    is trained and whose weight is frozen.  Y: bf16 [M, P], rows Y.stride(0) >= P apart.  Always the deterministic form: the kernel has no
    other.  ws: the caller's workspace of >= bias_grad_ws_floats(M, P) floats (tests); by default the stream's shared one."""
    if not Y.is_cuda or Y.dtype != torch.bfloat16 or Y.dim() != 2 or Y.stride(1) != 1:
        raise RuntimeError("Y: expected a bf16 [M, P] GPU tensor with unit column stride")
    _req(dbias, torch.float32, "dbias")
    M, P = Y.shape
    if dbias.numel() != P:
        raise ValueError("bias_grad: dbias holds P floats")
    lib = load()
    if ws is None:
        ws = _workspace(_ws_size(lib.dcv_bias_grad_ws_floats(M, P)), dbias)
    else:
        _req(ws, torch.float32, "ws")
    with _timer(lambda: ("bias_grad_kernel", f"M{M} P{P}", 0.0, None, 2.0 * M * P)):
        rc = lib.dcv_bias_grad(_p(Y), Y.stride(0), M, P, _p(dbias), _p(ws), ws.numel(), _stream())
    _check(rc, "dcv_bias_grad")


def dino_loss_ws_floats(V, B, K) -> int:
    return _ws_size(load().dcv_dino_loss_ws_floats(V, B, K))


def dino_loss_plan(V, B, K, aligned=True) -> dict:
    """The launch plan of dino_loss_fwd / dino_loss_bwd (include/dcv.h: dcv_dino_loss_plan) — host logic, callable without a GPU."""
    vec, tile_cols, col_tiles, wpw, grid, passes = (C.c_int() for _ in range(6))
    items = C.c_long()
    rc = load().dcv_dino_loss_plan(V, B, K, int(bool(aligned)), C.addressof(vec), C.addressof(tile_cols), C.addressof(col_tiles),
                                   C.addressof(items), C.addressof(wpw), C.addressof(grid), C.addressof(passes))
    _check(rc, "dcv_dino_loss_plan")
    return dict(vec=vec.value, tile_cols=tile_cols.value, col_tiles=col_tiles.value, items=items.value, waves_per_wg=wpw.value, grid=grid.value,
                passes=passes.value)


def _dino_operands(S, T, center, V):
    for t, name in ((S, "S"), (T, "T")):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: expected {torch.float32}, got {t.dtype}")
        if t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"{name}: expected a [rows, K] tensor with unit column stride")
    _req(center, torch.float32, "center")
    K = S.shape[1]
    if V < 2 or S.shape[0] % V or T.shape[0] % 2 or S.shape[0] // V != T.shape[0] // 2 or T.shape[1] != K or center.numel() != K:
        raise ValueError("dino_loss: S holds V*B rows of K logits (V >= 2), T 2*B rows of K, center K floats")
    return S.shape[0] // V, K


def dino_loss_fwd(S, T, center, V, student_temp, teacher_temp, loss, s_stats=None, t_stats=None, tsum=None, ws=None):
    """loss[0] = DINO's multi-crop loss of the student logits S [V*B, K] (view-major, views 0 and 1 global) against the teacher logits T [2*B, K]
    and the centre (include/dcv.h: dcv_dino_loss_fwd); rows S.stride(0) / T.stride(0) >= K apart.  s_stats [V*B, 2], t_stats [2*B, 3]: the row
    statistics dino_loss_bwd reads; tsum [K]: the column sums of T; each written unless None.  Always deterministic: the kernels have no other
    form.  ws: the caller's workspace of >= dino_loss_ws_floats(V, B, K) floats (tests); by default the stream's shared one."""
    B, K = _dino_operands(S, T, center, V)
    _req(loss, torch.float32, "loss")
    for t, name, n in ((s_stats, "s_stats", 2 * V * B), (t_stats, "t_stats", 6 * B), (tsum, "tsum", K)):
        if t is not None:
            _req(t, torch.float32, name)
            if t.numel() < n:
                raise ValueError(f"dino_loss_fwd: {name} holds {n} floats")
    lib = load()
    if ws is None:
        ws = _workspace(_ws_size(lib.dcv_dino_loss_ws_floats(V, B, K)), S)
    else:
        _req(ws, torch.float32, "ws")
    with _timer(lambda: ("dino_loss_fwd_kernel", f"V{V} B{B} K{K}", 0.0, None, 4.0 * K * (B * (V + 2 + (2 if tsum is not None else 0)) + 1))):
        rc = lib.dcv_dino_loss_fwd(_p(S), S.stride(0), _p(T), T.stride(0), _p(center), V, B, K, float(student_temp), float(teacher_temp), _p(loss),
                                   _p(s_stats), _p(t_stats), _p(tsum), _p(ws), ws.numel(), _stream())
    _check(rc, "dcv_dino_loss_fwd")


def dino_loss_bwd(S, T, center, V, student_temp, teacher_temp, s_stats, t_stats, g, dS):
    """dS [V*B, K] (rows dS.stride(0) >= K apart) = g[0] * d loss / d S from the statistics dino_loss_fwd saved (include/dcv.h: dcv_dino_loss_bwd);
    g: the incoming gradient, one float on the device."""
    B, K = _dino_operands(S, T, center, V)
    _req(s_stats, torch.float32, "s_stats"); _req(t_stats, torch.float32, "t_stats"); _req(g, torch.float32, "g")
    if not dS.is_cuda or dS.dtype != torch.float32 or dS.dim() != 2 or dS.stride(1) != 1 or dS.shape != S.shape:
        raise RuntimeError("dS: expected a float32 GPU tensor of S's shape with unit column stride")
    if s_stats.numel() < 2 * V * B or t_stats.numel() < 6 * B or g.numel() != 1:
        raise ValueError("dino_loss_bwd: s_stats holds 2*V*B floats, t_stats 6*B, g one")
    with _timer(lambda: ("dino_loss_bwd_kernel", f"V{V} B{B} K{K}", 0.0, None, 4.0 * K * (B * (2 * V + 2) + 1))):
        rc = load().dcv_dino_loss_bwd(_p(S), S.stride(0), _p(T), T.stride(0), _p(center), _p(s_stats), _p(t_stats), _p(g), V, B, K,
                                      float(student_temp), float(teacher_temp), _p(dS), dS.stride(0), _stream())
    _check(rc, "dcv_dino_loss_bwd")


def ibot_loss_ws_floats(R, K) -> int:
    return _ws_size(load().dcv_ibot_loss_ws_floats(R, K))


def ibot_loss_plan(R, K, aligned=True) -> dict:
    """The launch plan of ibot_loss_fwd / ibot_loss_bwd (include/dcv.h: dcv_ibot_loss_plan) — host logic, callable without a GPU."""
    vec, tile_cols, col_tiles, chunk_rows, chunks, wpw, grid, passes = (C.c_int() for _ in range(8))
    items = C.c_long()
    rc = load().dcv_ibot_loss_plan(R, K, int(bool(aligned)), C.addressof(vec), C.addressof(tile_cols), C.addressof(col_tiles),
                                   C.addressof(chunk_rows), C.addressof(chunks), C.addressof(items), C.addressof(wpw), C.addressof(grid),
                                   C.addressof(passes))
    _check(rc, "dcv_ibot_loss_plan")
    return dict(vec=vec.value, tile_cols=tile_cols.value, col_tiles=col_tiles.value, chunk_rows=chunk_rows.value, chunks=chunks.value,
                items=items.value, waves_per_wg=wpw.value, grid=grid.value, passes=passes.value)


def _ibot_operands(S, T, center, weights):
    for t, name in ((S, "S"), (T, "T")):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: expected {torch.float32}, got {t.dtype}")
        if t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"{name}: expected a [rows, K] tensor with unit column stride")
    _req(center, torch.float32, "center"); _req(weights, torch.float32, "weights")
    R, K = S.shape
    if R < 1 or T.shape != S.shape or center.numel() != K or weights.numel() != R:
        raise ValueError("ibot_loss: S and T hold R >= 1 rows of K logits, center K floats, weights R")
    return R, K


def ibot_loss_fwd(S, T, center, weights, student_temp, teacher_temp, loss, s_stats=None, t_stats=None, tsum=None, ws=None):
    """loss[0] = the masked patch-token distillation loss of the student logits S [R, K] against the teacher logits T [R, K] (row r of both the
    same token), the centre and the row weights (include/dcv.h: dcv_ibot_loss_fwd); rows S.stride(0) / T.stride(0) >= K apart.  s_stats [R, 3],
    t_stats [R, 4]: the row statistics ibot_loss_bwd reads; tsum [K]: the unweighted column sums of T; each written unless None.  Always
    deterministic: the kernels have no other form.  ws: the caller's workspace of >= ibot_loss_ws_floats(R, K) floats (tests); by default the
    stream's shared one."""
    R, K = _ibot_operands(S, T, center, weights)
    _req(loss, torch.float32, "loss")
    for t, name, n in ((s_stats, "s_stats", 3 * R), (t_stats, "t_stats", 4 * R), (tsum, "tsum", K)):
        if t is not None:
            _req(t, torch.float32, name)
            if t.numel() < n:
                raise ValueError(f"ibot_loss_fwd: {name} holds {n} floats")
    lib = load()
    if ws is None:
        ws = _workspace(_ws_size(lib.dcv_ibot_loss_ws_floats(R, K)), S)
    else:
        _req(ws, torch.float32, "ws")
    with _timer(lambda: ("ibot_loss_fwd_kernel", f"R{R} K{K}", 0.0, None, 4.0 * K * (2 * R + 1))):
        rc = lib.dcv_ibot_loss_fwd(_p(S), S.stride(0), _p(T), T.stride(0), _p(center), _p(weights), R, K, float(student_temp), float(teacher_temp),
                                   _p(loss), _p(s_stats), _p(t_stats), _p(tsum), _p(ws), ws.numel(), _stream())
    _check(rc, "dcv_ibot_loss_fwd")


def ibot_loss_bwd(S, T, center, weights, student_temp, teacher_temp, s_stats, t_stats, g, dS):
    """dS [R, K] (rows dS.stride(0) >= K apart) = g[0] * d loss / d S from the statistics ibot_loss_fwd saved (include/dcv.h: dcv_ibot_loss_bwd);
    g: the incoming gradient, one float on the device."""
    R, K = _ibot_operands(S, T, center, weights)
    _req(s_stats, torch.float32, "s_stats"); _req(t_stats, torch.float32, "t_stats"); _req(g, torch.float32, "g")
    if not dS.is_cuda or dS.dtype != torch.float32 or dS.dim() != 2 or dS.stride(1) != 1 or dS.shape != S.shape:
        raise RuntimeError("dS: expected a float32 GPU tensor of S's shape with unit column stride")
    if s_stats.numel() < 3 * R or t_stats.numel() < 4 * R or g.numel() != 1:
        raise ValueError("ibot_loss_bwd: s_stats holds 3*R floats, t_stats 4*R, g one")
    with _timer(lambda: ("ibot_loss_bwd_kernel", f"R{R} K{K}", 0.0, None, 4.0 * K * (3 * R + 1))):
        rc = load().dcv_ibot_loss_bwd(_p(S), S.stride(0), _p(T), T.stride(0), _p(center), _p(weights), _p(s_stats), _p(t_stats), _p(g), R, K,
                                      float(student_temp), float(teacher_temp), _p(dS), dS.stride(0), _stream())
    _check(rc, "dcv_ibot_loss_bwd")


def ln_fwd(x, gamma, beta, out, mean, rstd, M, D, eps, x_row_stride=None):
    with _timer(lambda: (f"ln_fwd_kernel<{'true' if out.dtype == torch.float32 else 'false'}, {2 if D <= 512 else 4}>", f"M{M} D{D}", 0.0, None,
                         M * D * (4.0 + (4.0 if out.dtype == torch.float32 else 2.0)))):
        rc = load().dcv_ln_fwd(_p(x), D if x_row_stride is None else x_row_stride, _p(gamma), _p(beta), _p(out),
                               1 if out.dtype == torch.float32 else 0, _p(mean), _p(rstd), M, D, eps, _stream())
    _check(rc, "dcv_ln_fwd")


def ln_pool_channels(x, gamma, beta, out, B, C, n_p, D, eps, ws=None):
    """out [B, 1 + C, D] fp32 = LayerNorm of x [B, 1 + C * n_p, D] pooled per channel: row 0 the normed CLS row, row 1 + c the mean of the normed
    patch rows of channel c (include/dcv.h: dcv_ln_pool_channels).  ws: the caller's workspace (tests); by default the stream's shared one."""
    _req(x, torch.float32, "x"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta"); _req(out, torch.float32, "out")
    if x.numel() < B * (1 + C * n_p) * D or out.numel() < B * (1 + C) * D or gamma.numel() < D or beta.numel() < D:
        raise ValueError("ln_pool_channels: x holds B*(1+C*n_p)*D floats, out B*(1+C)*D, gamma and beta D")
    lib = load()
    with _timer(lambda: (f"ln_pool_kernel<{2 if D <= 512 else 4}>", f"B{B} C{C} n{n_p} D{D}", 0.0, None, 4.0 * D * B * (2 + C * n_p + C))):
        if ws is None:
            need = _ws_size(lib.dcv_ln_pool_channels_ws_floats(B, C, n_p, D))
            ws = _workspace(need, out) if need else None
        else:
            _req(ws, torch.float32, "ws")
        rc = lib.dcv_ln_pool_channels(_p(x), _p(gamma), _p(beta), float(eps), _p(out), B, C, n_p, D, _p(ws), ws.numel() if ws is not None else 0,
                                      _stream())
    _check(rc, "dcv_ln_pool_channels")


def ln_pool_channels_bwd(x, gamma, dout, dx, dgamma, dbeta, B, C, n_p, D, eps, ws=None):
    """Adjoint of ln_pool_channels: dx [B, 1 + C * n_p, D] += the gradient of the pooled LayerNorm for dout [B, 1 + C, D]; dgamma / dbeta [D]
    (each may be None) accumulated (include/dcv.h: dcv_ln_pool_channels_bwd).  Always the deterministic form: the kernel has no
    other.  ws: the caller's workspace (tests); by default the stream's shared one."""
    _req(x, torch.float32, "x"); _req(gamma, torch.float32, "gamma"); _req(dout, torch.float32, "dout"); _req(dx, torch.float32, "dx")
    if x.numel() < B * (1 + C * n_p) * D or dx.numel() < B * (1 + C * n_p) * D or dout.numel() < B * (1 + C) * D or gamma.numel() < D:
        raise ValueError("ln_pool_channels_bwd: x and dx hold B*(1+C*n_p)*D floats, dout B*(1+C)*D, gamma D")
    for t, name in ((dgamma, "dgamma"), (dbeta, "dbeta")):
        if t is not None:
            _req(t, torch.float32, name)
            if t.numel() < D:
                raise ValueError(f"ln_pool_channels_bwd: {name} holds D floats")
    lib = load()
    with _timer(lambda: (f"ln_pool_bwd_kernel<{2 if D <= 512 else 4}>", f"B{B} C{C} n{n_p} D{D}", 0.0, None, 4.0 * D * B * (3 * (1 + C * n_p) + 1 + C))):
        if ws is None:
            ws = _workspace(_ws_size(lib.dcv_ln_pool_channels_bwd_ws_floats(B, C, n_p, D)), dx) if dgamma is not None else None
        else:
            _req(ws, torch.float32, "ws")
        rc = lib.dcv_ln_pool_channels_bwd(_p(x), _p(gamma), float(eps), _p(dout), _p(dx), _p(dgamma), _p(dbeta), B, C, n_p, D, _p(ws),
                                          ws.numel() if ws is not None else 0, _stream())
    _check(rc, "dcv_ln_pool_channels_bwd")


def ln_bwd(du, x, mean, rstd, gamma, dx_in, dx_out, dx_bf16, dgamma, dbeta, M, D, x_row_stride=None, dx_row_stride=None,
           bf16_row_scale=None, rows_per_sample=1):
    """bf16_row_scale [M / rows_per_sample] (fp32): dx_bf16 = bf16(scale[row / rows_per_sample] * dx_out) (DropPath, dcv_ln_bwd_scaled)."""
    with _timer(lambda: (f"ln_bwd_kernel<{'true' if du.dtype == torch.float32 else 'false'}, {2 if D <= 512 else 4}>", f"M{M} D{D}", 0.0, None,
                         M * D * ((4.0 if du.dtype == torch.float32 else 2.0) + 4.0 + (4.0 if dx_in is not None else 0.0) + 4.0 + (2.0 if dx_bf16 is not None else 0.0)))):
        lib = load()
        args = (_p(du), 1 if du.dtype == torch.float32 else 0, _p(x), D if x_row_stride is None else x_row_stride,
                _p(mean), _p(rstd), _p(gamma), _p(dx_in), _p(dx_out), D if dx_row_stride is None else dx_row_stride,
                _p(dx_bf16), _p(dgamma), _p(dbeta), M, D)
        ws = _workspace(_ws_size(lib.dcv_ln_bwd_det_ws_floats(M, D)), dx_out) if _deterministic else None
        if bf16_row_scale is not None:
            _req(bf16_row_scale, torch.float32, "bf16_row_scale")
            rc = lib.dcv_ln_bwd_scaled(*args, _p(bf16_row_scale), rows_per_sample, _p(ws), ws.numel() if ws is not None else 0, _stream())
        elif ws is not None:
            rc = lib.dcv_ln_bwd_det(*args, _p(ws), ws.numel(), _stream())
        else:
            rc = lib.dcv_ln_bwd(*args, _stream())
    _check(rc, "dcv_ln_bwd")


def attn_fwd(qkv, o, lse, B, N, H, hd, scale, nq=None, prescaled=False):
    """nq: only the query rows [0, nq) of every (batch, head) are processed (default: all N).
    prescaled: the q part of qkv holds q * scale * log2(e) (dcv_attn_fwd_rows_ps)."""
    nq_ = N if nq is None else nq
    prod = 2.0 * B * H * nq_ * N * hd  # one (query rows) x N x head_dim product over all (batch, head) pairs
    D_ = H * hd
    with _timer(lambda: (f"attn_fwd3_kernel<{'true' if prescaled else 'false'}>", f"B{B} N{N} H{H} Nq{nq_}", 2 * prod, 2 * prod, 2.0 * B * (N * 2 * D_ + nq_ * 2 * D_) + 4.0 * B * H * nq_)):
        if prescaled:
            rc = load().dcv_attn_fwd_rows_ps(_p(qkv), _p(o), _p(lse), B, N, N if nq is None else nq, H, hd, _stream())
        else:
            rc = load().dcv_attn_fwd_rows(_p(qkv), _p(o), _p(lse), B, N, N if nq is None else nq, H, hd, scale, _stream())
    _check(rc, "dcv_attn_fwd")


def attn_bwd(qkv, o, dO, lse, delta_ws, dqkv, B, N, H, hd, scale, nq=None, prescaled=False):
    lib = load()
    dq_fn = lib.dcv_attn_bwd_dq_rows_ps if prescaled else lib.dcv_attn_bwd_dq_rows
    dkdv_fn = lib.dcv_attn_bwd_dkdv_rows_ps if prescaled else lib.dcv_attn_bwd_dkdv_rows
    nq = N if nq is None else nq
    if delta_ws.numel() < 2 * B * H * N or delta_ws.dtype != torch.float32:
        raise ValueError("attention backward workspace: 2*B*H*N float32 (-delta, then lse*log2e)")
    prod = 2.0 * B * H * nq * N * hd
    D_ = H * hd
    # algorithmic credit: the backward is 4 products (dP, dV, dK, dQ); the S recomputation is executed
    # in both kernels but not credited: dQ kernel 1 credited / 3 executed, dK/dV kernel 3 credited / 4 executed
    tp = "<true>" if prescaled else "<false>"  # the symbols as rocprofv3 prints them (the kernels are templates on the pre-scaled-q form)
    with _timer(lambda: ("attn_bwd_dq2_kernel" + tp, f"B{B} N{N} H{H} Nq{nq}", 1 * prod, 3 * prod, 2.0 * B * (N * 3 * D_ + nq * 3 * D_))):  # also writes the row statistics
        rc = dq_fn(_p(qkv), _p(o), _p(dO), _p(lse), _p(delta_ws), _p(dqkv), B, N, nq, H, hd, scale, _stream())
    _check(rc, "dcv_attn_bwd_dq")
    # pre-scaled q: the persistent third form (csrc/attn_bwd3.hip) + the second form's launch for a key remainder < 129; plain: the second form
    with _timer(lambda: (("attn_bwd_dkdv3p_kernel" if prescaled else "attn_bwd_dkdv2_kernel<false>"), f"B{B} N{N} H{H} Nq{nq}", 3 * prod, 4 * prod, 2.0 * B * (N * 3 * D_ + nq * 1 * D_ + N * 2 * D_))):
        rc = dkdv_fn(_p(qkv), _p(dO), _p(lse), _p(delta_ws), _p(dqkv), B, N, nq, H, hd, scale, _stream())
    _check(rc, "dcv_attn_bwd_dkdv")


def attn_probs(qkv, lse, P, B, N, H, hd, scale, nq=None, prescaled=False):
    """P [B, H, nq, N] fp32 = softmax(q k^T * scale) of the query rows [0, nq) (default: all N) from qkv and the forward's lse
    (include/dcv.h: dcv_attn_probs_rows).  prescaled: the q part of qkv holds q * scale * log2(e) (dcv_attn_probs_rows_ps; scale unused)."""
    _req(qkv, torch.bfloat16, "qkv"); _req(lse, torch.float32, "lse"); _req(P, torch.float32, "P")
    nq_ = N if nq is None else nq
    if P.numel() < B * H * nq_ * N or lse.numel() < B * H * N:
        raise ValueError("attn_probs: P holds B*H*nq*N floats, lse B*H*N")
    with _timer(lambda: (f"attn_probs_kernel<{'true' if prescaled else 'false'}>", f"B{B} N{N} H{H} Nq{nq_}", 2.0 * B * H * nq_ * N * hd, None,
                         4.0 * B * H * nq_ * N)):
        if prescaled:
            rc = load().dcv_attn_probs_rows_ps(_p(qkv), _p(lse), _p(P), B, N, nq_, H, hd, _stream())
        else:
            rc = load().dcv_attn_probs_rows(_p(qkv), _p(lse), _p(P), B, N, nq_, H, hd, float(scale), _stream())
    _check(rc, "dcv_attn_probs_rows")


def attn_channel_mass(qkv, lse, B, N, H, hd, scale, C, n_p, tok=None, ch=None, prescaled=False, ws=None):
    """The attention of one block reduced to channel granularity, from qkv and the forward's lse (include/dcv.h: dcv_attn_channel_mass): with the key
    segments S_0 = {CLS}, S_{1+c} = the n_p tokens of channel c (N = 1 + C * n_p), tok [B, H, N, 1 + C] fp32 = the mass each query puts on each
    segment and ch [B, H, 1 + C, 1 + C] fp32 = its mean over the queries of each segment.  Either may be None, not both.  prescaled: as attn_probs.
    ws: the caller's workspace (tests), read only for ch without tok; by default the stream's shared one."""
    _req(qkv, torch.bfloat16, "qkv"); _req(lse, torch.float32, "lse")
    if tok is None and ch is None:
        raise ValueError("attn_channel_mass: tok and ch are both None")
    if tok is not None:
        _req(tok, torch.float32, "tok")
    if ch is not None:
        _req(ch, torch.float32, "ch")
    if qkv.numel() < B * N * 3 * H * hd or lse.numel() < B * H * N or (tok is not None and tok.numel() < B * H * N * (1 + C)) or \
            (ch is not None and ch.numel() < B * H * (1 + C) * (1 + C)):
        raise ValueError("attn_channel_mass: qkv holds B*N*3*H*hd elements, lse B*H*N floats, tok B*H*N*(1+C), ch B*H*(1+C)*(1+C)")
    lib = load()
    with _timer(lambda: (f"attn_channel_mass_kernel<{'true' if prescaled else 'false'}>", f"B{B} N{N} H{H} C{C} n{n_p}", 2.0 * B * H * N * N * hd, None,
                         2.0 * B * N * 2 * H * hd + 4.0 * B * H * N * (2 + C))):
        if ws is None:
            if ch is not None and tok is None:
                ws = _workspace(_ws_size(lib.dcv_attn_channel_mass_ws_floats(B, N, H, C)), ch)
        else:
            _req(ws, torch.float32, "ws")
        nws = ws.numel() if ws is not None else 0
        if prescaled:
            rc = lib.dcv_attn_channel_mass_ps(_p(qkv), _p(lse), _p(tok), _p(ch), B, N, H, hd, C, n_p, _p(ws), nws, _stream())
        else:
            rc = lib.dcv_attn_channel_mass(_p(qkv), _p(lse), _p(tok), _p(ch), B, N, H, hd, float(scale), C, n_p, _p(ws), nws, _stream())
    _check(rc, "dcv_attn_channel_mass")


def attn_rollout_step(qkv, lse, w, out, B, N, H, hd, scale, alpha, prescaled=False):
    """One attention-rollout step over one block, heads averaged, from qkv and the forward's lse (include/dcv.h: dcv_attn_rollout_step):
    out [B, N] fp32 = w^T (alpha I + (1 - alpha) mean_h P) for w [B, N] fp32 >= 0.  out must not overlap w; alpha in [0, 1).  prescaled: as
    attn_probs."""
    _req(qkv, torch.bfloat16, "qkv"); _req(lse, torch.float32, "lse"); _req(w, torch.float32, "w"); _req(out, torch.float32, "out")
    if qkv.numel() < B * N * 3 * H * hd or lse.numel() < B * H * N or w.numel() < B * N or out.numel() < B * N:
        raise ValueError("attn_rollout_step: qkv holds B*N*3*H*hd elements, lse B*H*N floats, w and out B*N")
    with _timer(lambda: (f"attn_keysweep_kernel<{'true' if prescaled else 'false'}, false>", f"B{B} N{N} H{H}", 2.0 * B * H * N * N * hd, None,
                         2.0 * B * N * 2 * H * hd + 4.0 * B * N * (H + 2))):
        if prescaled:
            rc = load().dcv_attn_rollout_step_ps(_p(qkv), _p(lse), _p(w), _p(out), B, N, H, hd, float(alpha), _stream())
        else:
            rc = load().dcv_attn_rollout_step(_p(qkv), _p(lse), _p(w), _p(out), B, N, H, hd, float(scale), float(alpha), _stream())
    _check(rc, "dcv_attn_rollout_step")


def attn_relevance_step(qkv, lse, dO, w, out, B, N, H, hd, scale, nq=None, prescaled=False):
    """One step of gradient-weighted attention relevance over one block, heads averaged, from qkv, the forward's lse and the gradient dO
    [B, N, H * hd] bf16 with respect to the attention output (include/dcv.h: dcv_attn_relevance_step):
    out [B, N] fp32 = w + w^T mean_h relu(dP . P) over the query rows [0, nq) (default: all N), dP = dO V^T, for w [B, N] fp32 >= 0.  out must
    not overlap w.  prescaled: as attn_probs."""
    _req(qkv, torch.bfloat16, "qkv"); _req(lse, torch.float32, "lse"); _req(dO, torch.bfloat16, "dO"); _req(w, torch.float32, "w")
    _req(out, torch.float32, "out")
    nq_ = N if nq is None else nq
    if qkv.numel() < B * N * 3 * H * hd or lse.numel() < B * H * N or dO.numel() < B * N * H * hd or w.numel() < B * N or out.numel() < B * N:
        raise ValueError("attn_relevance_step: qkv holds B*N*3*H*hd elements, lse B*H*N floats, dO B*N*H*hd elements, w and out B*N")
    with _timer(lambda: (f"attn_keysweep_kernel<{'true' if prescaled else 'false'}, true>", f"B{B} N{N} H{H} Nq{nq_}", 4.0 * B * H * nq_ * N * hd, None,
                         2.0 * B * (N * 2 + nq_ * 2) * H * hd + 4.0 * B * (nq_ * (H + 1) + 2 * N))):
        if prescaled:
            rc = load().dcv_attn_relevance_step_ps(_p(qkv), _p(lse), _p(dO), _p(w), _p(out), B, N, nq_, H, hd, _stream())
        else:
            rc = load().dcv_attn_relevance_step(_p(qkv), _p(lse), _p(dO), _p(w), _p(out), B, N, nq_, H, hd, float(scale), _stream())
    _check(rc, "dcv_attn_relevance_step")


def im2col(x, ch_idx, out, B, Ct, C, H, W, P, scale=None, shift=None):
    if x.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError(f"x: expected float32 or uint8 images, got {x.dtype}")
    _req(x, x.dtype, "x"); _req(ch_idx, torch.int32, "ch_idx")
    _check(load().dcv_im2col_bf16(_p(x), 1 if x.dtype == torch.uint8 else 0, _p(ch_idx), _p(scale), _p(shift), _p(out), B, Ct, C, H, W,
                                  P, _stream()), "dcv_im2col_bf16")


def patch_dgrad(dY, W, ch_idx, dx, B, Ct, C, H, Wimg, P, scale=None):
    """dx [B, Ct, H, W] f32 = the input-image gradient of the tokeniser (include/dcv.h: dcv_patch_dgrad): dY [B*C*n, D] bf16 token gradients,
    W [D, P*P] bf16 the projection operand the forward used, ch_idx int32 [C], scale f32 [C] (the input affine's, or None).  Every element of dx
    is written; unsupported shapes (P not 8 / 16, D not 192 / 384 / 768) raise."""
    _req(dY, torch.bfloat16, "dY"); _req(W, torch.bfloat16, "W"); _req(ch_idx, torch.int32, "ch_idx"); _req(dx, torch.float32, "dx")
    if scale is not None:
        _req(scale, torch.float32, "scale")
    D = W.shape[0]
    n = (H // P) * (Wimg // P)
    if W.numel() != D * P * P or dY.shape != (B * C * n, D) or dx.numel() != B * Ct * H * Wimg or ch_idx.numel() != C:
        raise ValueError("patch_dgrad: dY [B*C*n, D], W [D, P*P], ch_idx [C], dx [B, Ct, H, W]")
    with _timer(lambda: (f"patch_dgrad_kernel<{P}, {D}>", f"M{B * C * n} D{D} P{P}", 2.0 * B * C * n * D * P * P, None,
                         2.0 * B * C * n * D + 4.0 * B * Ct * H * Wimg)):
        rc = load().dcv_patch_dgrad(_p(dY), _p(W), _p(ch_idx), _p(scale), _p(dx), B, Ct, C, H, Wimg, P, D, _stream())
    _check(rc, "dcv_patch_dgrad")


def patch_bwd(dx0, dYloss, dY_bf16, dE, dpos, dcls, B, C, n, D):
    lib = load()
    if _deterministic:
        ws = _workspace(_ws_size(lib.dcv_patch_bwd_det_ws_floats(B, C, n, D)), dx0)
        rc = lib.dcv_patch_bwd_det(_p(dx0), _p(dYloss), _p(dY_bf16), _p(dE), _p(dpos), _p(dcls), B, C, n, D, _p(ws), ws.numel(), _stream())
    else:
        rc = lib.dcv_patch_bwd(_p(dx0), _p(dYloss), _p(dY_bf16), _p(dE), _p(dpos), _p(dcls), B, C, n, D, _stream())
    _check(rc, "dcv_patch_bwd")


def _mask_arg(mask, B, C, n):
    if not mask.is_cuda or mask.dtype not in (torch.uint8, torch.bool) or not mask.is_contiguous() or mask.numel() != B * C * n:
        raise RuntimeError("mask: expected a contiguous uint8 or bool GPU tensor [B, C * n]")
    return mask


def mask_tokens_fwd(xs, mask, mask_token, E, pos, B, C, n, D):
    """xs [B, 1 + C n, D]: the masked token rows (mask uint8 [B, C n] != 0) become mask_token + (E[c] + pos[1 + i]), the EPI_PATCH epilogue's
    bits for a projection output of mask_token (include/dcv.h: dcv_mask_tokens_fwd).  Nothing else is written."""
    for t, name in ((xs, "xs"), (mask_token, "mask_token"), (E, "E"), (pos, "pos")):
        _req(t, torch.float32, name)
    if xs.numel() != B * (1 + C * n) * D or mask_token.numel() != D or E.numel() < C * D or pos.numel() < (1 + n) * D:
        raise ValueError("mask_tokens_fwd: xs holds B (1 + C n) D floats, mask_token D, E C D, pos (1 + n) D")
    _mask_arg(mask, B, C, n)
    with _timer(lambda: ("mask_tokens_fwd_kernel", f"B{B} C{C} n{n} D{D}", 0.0, None, 1.0 * B * C * n)):
        rc = load().dcv_mask_tokens_fwd(_p(xs), _p(mask), _p(mask_token), _p(E), _p(pos), B, C, n, D, _stream())
    _check(rc, "dcv_mask_tokens_fwd")


def mask_tokens_bwd(dx0, mask, dYloss, dY_bf16, dmask_token, B, C, n, D, ws=None):
    """After patch_bwd: dmask_token [D] += the masked rows' dx0[b, 1 + t, :]; the masked rows of dY_bf16 [B C n, D] become bf16(dYloss row), or 0
    when dYloss is None (include/dcv.h: dcv_mask_tokens_bwd).  No atomics in either reduction mode: partials through the workspace."""
    _req(dx0, torch.float32, "dx0"); _req(dY_bf16, torch.bfloat16, "dY_bf16"); _req(dmask_token, torch.float32, "dmask_token")
    if dYloss is not None:
        _req(dYloss, torch.float32, "dYloss")
    if (dx0.numel() != B * (1 + C * n) * D or dY_bf16.numel() != B * C * n * D or dmask_token.numel() != D
            or (dYloss is not None and dYloss.numel() != B * C * n * D)):
        raise ValueError("mask_tokens_bwd: dx0 holds B (1 + C n) D floats, dY_bf16 and dYloss B C n D, dmask_token D")
    _mask_arg(mask, B, C, n)
    lib = load()
    if ws is None:
        ws = _workspace(_ws_size(lib.dcv_mask_tokens_bwd_ws_floats(B, C, n, D)), dx0)
    else:
        _req(ws, torch.float32, "ws")
    with _timer(lambda: ("mask_tokens_bwd_kernel", f"B{B} C{C} n{n} D{D}", 0.0, None, 1.0 * B * C * n)):
        rc = lib.dcv_mask_tokens_bwd(_p(dx0), _p(mask), _p(dYloss), _p(dY_bf16), _p(dmask_token), B, C, n, D, _p(ws), ws.numel(), _stream())
    _check(rc, "dcv_mask_tokens_bwd")


def gather_tokens(x, idx, out, B, N, Nk, D, scatter=False):
    _check(load().dcv_gather_tokens(_p(x), _p(idx), _p(out), B, N, Nk, D, 1 if scatter else 0, _stream()), "dcv_gather_tokens")


def fill_cls(x, cls, pos0, B, batch_stride, D):
    _check(load().dcv_fill_cls(_p(x), _p(cls), _p(pos0), B, batch_stride, D, _stream()), "dcv_fill_cls")


TPS_MIN_W, TPS_MAX_W, TPS_MAX_K, CROP_MAX_SCALE = 21, 1024, 32, 8


def _images(x, name):
    """Shape and dtype of a raw image batch, checked before anything touches the device: (B, C, H, W)."""
    if x.dim() != 4:
        raise ValueError(f"{name}: expected images [B, C, H, W], got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name}: expected float32 or uint8 images, got {x.dtype}")
    return tuple(x.shape)


def tps_warp(x, P, coef, apply, out):
    """out[b] f32 = the reference's thin-plate-spline warp of x[b] for the samples with apply[b] != 0 (include/dcv.h: dcv_tps_warp); the other
    samples of out are not written.  x [B, C, W, W] uint8 / float32, P f64 [B, K, 2], coef f64 [B, 2, K + 3], apply int32 [B]."""
    B, C, H, W = _images(x, "tps_warp: x")
    if H != W:
        raise ValueError(f"tps_warp: square images only (the reference's corner points mix width and height otherwise), got {H} x {W}")
    if not TPS_MIN_W <= W <= TPS_MAX_W:
        raise ValueError(f"tps_warp: {TPS_MIN_W} <= W <= {TPS_MAX_W}, got {W}")
    K = P.shape[1] if P.dim() == 3 else 0
    if not 1 <= K <= TPS_MAX_K or P.shape != (B, K, 2) or coef.shape != (B, 2, K + 3) or apply.shape != (B,) or out.shape != x.shape:
        raise ValueError(f"tps_warp: P [B, K <= {TPS_MAX_K}, 2], coef [B, 2, K + 3], apply [B], out like x")
    _req(x, x.dtype, "x"); _req(P, torch.float64, "P"); _req(coef, torch.float64, "coef"); _req(apply, torch.int32, "apply"); _req(out, torch.float32, "out")
    with _timer(lambda: (f"tps_warp_kernel<{'uint8_t' if x.dtype == torch.uint8 else 'float'}>", f"B{B} C{C} W{W}", 0.0, None,
                         float(B * C * W * W * (x.element_size() + 4)))):  # all samples flagged
        rc = load().dcv_tps_warp(_p(x), 1 if x.dtype == torch.uint8 else 0, _p(P), _p(coef), _p(apply), _p(out), B, C, W, K, _stream())
    _check(rc, "dcv_tps_warp")


def check_crop_boxes(box, H, W, S):
    """box: host int [B, 4] rows (i, j, h, w).  ValueError for a box outside the H x W image or one that shrinks by more than 8 on an axis."""
    for i, j, h, w in box.tolist():
        if h < 1 or w < 1 or i < 0 or j < 0 or i + h > H or j + w > W:
            raise ValueError(f"crop box (i={i}, j={j}, h={h}, w={w}) leaves the {H} x {W} image")
        if h > CROP_MAX_SCALE * S or w > CROP_MAX_SCALE * S:
            raise ValueError(f"crop box {h} x {w} -> {S}: scale > {CROP_MAX_SCALE} is not supported")


def crop_resize_flip(x, warped, use_warped, box, flip, out):
    """out f32 [B, C, S, S] = box[b] of (warped[b] if use_warped[b] else x[b]) resized as torch's antialiased bilinear interpolate, mirrored where
    flip[b] (include/dcv.h: dcv_crop_resize_flip); warped None: all from x.  box int32 [B, 4] ON THE DEVICE: check_crop_boxes() is for its host copy."""
    B, C, H, W = _images(x, "crop_resize_flip: x")
    if out.dim() != 4 or out.shape[:2] != (B, C) or out.shape[2] != out.shape[3]:
        raise ValueError("crop_resize_flip: out [B, C, S, S]")
    S = out.shape[2]
    if (warped is not None and (warped.shape != x.shape or use_warped.shape != (B,))) or flip.shape != (B,) or box.shape != (B, 4):
        raise ValueError("crop_resize_flip: warped like x, use_warped [B], box [B, 4], flip [B]")
    _req(x, x.dtype, "x"); _req(box, torch.int32, "box")
    if warped is None:
        use_warped = None  # every sample is read from x
    else:
        _req(warped, torch.float32, "warped"); _req(use_warped, torch.int32, "use_warped")
    _req(flip, torch.int32, "flip"); _req(out, torch.float32, "out")
    with _timer(lambda: (f"crop_resize_flip_kernel<{'uint8_t' if x.dtype == torch.uint8 else 'float'}>", f"B{B} C{C} H{H} W{W} S{S}", 0.0, None,
                         float(B * C * (H * W * x.element_size() + S * S * 4)))):  # whole-image boxes, nothing warped
        rc = load().dcv_crop_resize_flip(_p(x), 1 if x.dtype == torch.uint8 else 0, _p(warped), _p(use_warped), _p(box), _p(flip), _p(out), B, C, H, W, S,
                                         _stream())
    _check(rc, "dcv_crop_resize_flip")


def ortho_fwd(Y, S, selfsq, tot, inv_norm, stats, B, Cc, n, D):
    lib = load()
    if _deterministic:
        ws = _workspace(_ws_size(lib.dcv_ortho_fwd_det_ws_floats(B, Cc, n, D)), Y)
        rc = lib.dcv_ortho_fwd_det(_p(Y), _p(S), _p(selfsq), _p(tot), _p(inv_norm), _p(stats), B, Cc, n, D, _p(ws), ws.numel(), _stream())
    else:
        rc = lib.dcv_ortho_fwd(_p(Y), _p(S), _p(selfsq), _p(tot), _p(inv_norm), _p(stats), B, Cc, n, D, _stream())
    _check(rc, "dcv_ortho_fwd")


def ortho_bwd(Y, S, tot, inv_norm, coef, dY, B, Cc, n, D):
    _check(load().dcv_ortho_bwd(_p(Y), _p(S), _p(tot), _p(inv_norm), _p(coef), _p(dY), B, Cc, n, D, _stream()), "dcv_ortho_bwd")


def adamw(p, g, m, v, n, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    _check(load().dcv_adamw(_p(p), _p(g), _p(m), _p(v), n, lr, b1, b2, eps, wd, step, grad_scale, _stream()), "dcv_adamw")


def adamw_dyn(p, g, m, v, n, hyper_dev):
    _check(load().dcv_adamw_dyn(_p(p), _p(g), _p(m), _p(v), n, _p(hyper_dev), _stream()), "dcv_adamw_dyn")


def adamw_set_hyper(hyper_dev, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    _check(load().dcv_adamw_set_hyper(_p(hyper_dev), lr, b1, b2, eps, wd, step, grad_scale, _stream()), "dcv_adamw_set_hyper")


ADAMW_MAX_GROUPS, ADAMW_MAX_SEGS = 32, 1024  # include/dcv.h DCV_ADAMW_MAX_GROUPS / DCV_ADAMW_MAX_SEGS


def adamw_set_hyper_groups(hyper_dev, rows, steps, grad_scale=1.0):
    """rows: per group (lr, b1, b2, eps, wd); steps: per group step count (>= 1).  Host lists: they travel by value."""
    n = len(rows)
    r = (C.c_float * (5 * n))(*[float(x) for row in rows for x in row])
    s = (C.c_int * n)(*[int(x) for x in steps])
    _check(load().dcv_adamw_set_hyper_groups(_p(hyper_dev), C.cast(r, C.c_void_p), C.cast(s, C.c_void_p), n, grad_scale, _stream()),
           "dcv_adamw_set_hyper_groups")


def adamw_groups(p, g, m, v, n, seg_end4, seg_group, n_seg, hyper_dev, n_groups):
    _check(load().dcv_adamw_groups(_p(p), _p(g), _p(m), _p(v), n, _p(seg_end4), _p(seg_group), n_seg, _p(hyper_dev), n_groups, _stream()),
           "dcv_adamw_groups")


AVG_SWA, AVG_EMA = 0, 1  # include/dcv.h DCV_AVG_*


def avg_update(avg, p, n, mode, ema_weight=0.0, n_averaged=0, n_averaged_dev=None, grid_cap=0):
    """avg[:n] <- lerp(avg[:n], p[:n], w) in one launch (include/dcv.h: dcv_avg_update).  n_averaged_dev: an int64 device word holding the
    count of updates so far (read, never written); without it the count is n_averaged."""
    _req(avg, torch.float32, "avg"); _req(p, torch.float32, "p")
    if avg.numel() < n or p.numel() < n:
        raise ValueError("avg_update: avg and p hold at least n floats")
    if n_averaged_dev is not None:
        _req(n_averaged_dev, torch.int64, "n_averaged_dev")
    with _timer(lambda: ("avg_update_kernel", f"n{n}", 0.0, None, 12.0 * n)):
        rc = load().dcv_avg_update(_p(avg), _p(p), n, int(mode), float(ema_weight), int(n_averaged), _p(n_averaged_dev), int(grid_cap), _stream())
    _check(rc, "dcv_avg_update")


def cast_bf16(src, dst, n):
    _check(load().dcv_cast_bf16(_p(src), _p(dst), n, _stream()), "dcv_cast_bf16")


def cast_transpose_bf16(src_base, dst_base, desc_dev, n_desc, max_tiles):
    _check(load().dcv_cast_transpose_bf16(_p(src_base), _p(dst_base), _p(desc_dev), n_desc, max_tiles, _stream()), "dcv_cast_transpose_bf16")


def sumsq_acc(x, n, acc):
    lib = load()
    if _deterministic:
        ws = _workspace(_ws_size(lib.dcv_sumsq_det_ws_floats(n)), x)
        rc = lib.dcv_sumsq_acc_det(_p(x), n, _p(acc), _p(ws), ws.numel(), _stream())
    else:
        rc = lib.dcv_sumsq_acc(_p(x), n, _p(acc), _stream())
    _check(rc, "dcv_sumsq_acc")


def clip_scale(x, n, sumsq_dev, max_norm):
    _check(load().dcv_clip_scale(_p(x), n, _p(sumsq_dev), float(max_norm), _stream()), "dcv_clip_scale")


def cast_bf16_sr(src, dst, n, seed_dev):
    _check(load().dcv_cast_bf16_sr(_p(src), _p(dst), n, _p(seed_dev), _stream()), "dcv_cast_bf16_sr")


def cast_transpose_bf16_sr(src_base, dst_base, desc_dev, n_desc, max_tiles, seed_dev):
    _check(load().dcv_cast_transpose_bf16_sr(_p(src_base), _p(dst_base), _p(desc_dev), n_desc, max_tiles, _p(seed_dev), _stream()),
           "dcv_cast_transpose_bf16_sr")


def cast_scaled_ranges(src_base, dst_bf16, dst_f32, desc_dev, n_desc, blocks_per_desc, scale, seed_dev=None):
    """desc_dev int64 [n_desc][5] = {src offset, dst offset, count, scaled_count, kind (0: bf16 copy, 1: fp32 copy)} (dcv_cast_scaled_ranges)."""
    _check(load().dcv_cast_scaled_ranges(_p(src_base), _p(dst_bf16), _p(dst_f32), _p(desc_dev), n_desc, blocks_per_desc, float(scale),
                                         _p(seed_dev), _stream()), "dcv_cast_scaled_ranges")


def proxy_loss_supported(C: int, D: int) -> bool:
    return bool(load().dcv_proxy_loss_supported(C, D))


def proxy_loss(emb, proxies, scale: float, loss, d_emb, d_proxies):
    """loss[0] = CE(-cdist(scale * normalize(emb), scale * normalize(proxies))^2, eye(C)); d_emb / d_proxies = its gradients (dcv_proxy_loss)."""
    _req(emb, torch.float32, "emb"); _req(proxies, torch.float32, "proxies")
    C_, D_ = emb.shape
    if proxies.shape != emb.shape or not emb.is_contiguous() or not proxies.is_contiguous():
        raise ValueError("proxy_loss: emb and proxies are contiguous [C, D] fp32 tensors of the same shape")
    _check(load().dcv_proxy_loss(_p(emb), _p(proxies), C_, D_, float(scale), _p(loss), _p(d_emb), _p(d_proxies), _stream()), "dcv_proxy_loss")

