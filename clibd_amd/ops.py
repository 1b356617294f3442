"""Tensor-level wrappers over the C ABI (include/clibd_hip.h and the additive headers beside it).

PyTorch is plumbing here: it owns device memory and the HIP stream; every function below only checks the
operands on the host, takes raw pointers and enqueues hand-written gfx950 kernels on torch's current stream.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import torch

from . import _lib
from ._lib import GemmEpilogue, check

ACT_NONE, ACT_GELU, ACT_GELU_GRAD, ACT_GELU_SAVE_GRAD, ACT_MUL_AUX, ACT_ADD_AUX, ACT_GELU_SAVE_GRAD_U8, ACT_MUL_AUX_U8 = 0, 1, 2, 3, 4, 5, 6, 7
ACT_GELU_SAVE_GRAD_E12, ACT_MUL_AUX_E12 = 8, 9   # gelu' as the 12-bit e4m7 form of its bf16 value: uint8 buffers [M, 3N/2] (include/clibd_hip.h)
BF16, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32
FP8 = torch.float8_e4m3fn  # OCP e4m3 (gfx950's fp8 MFMA operand format); max finite 448


def _stream() -> int:
    """Raw handle of torch's current HIP stream.  Two direct C calls: `torch.cuda.current_stream().cuda_stream` builds a Stream object
    through four Python layers (8 us per call, 1.8 ms per step at ~1000 launches: tools/host_profile.py, round 4)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, name: str, contiguous: bool = True) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (clibd_amd has no CPU compute path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")


def _rowmajor(t: torch.Tensor, name: str) -> int:
    """2-D row-major view with unit inner stride; returns the leading dimension in elements."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a 2-D tensor with unit inner stride")
    return t.stride(0)


class Drop:
    """Dropout site: probability p and a 32-bit seed; the mask is hash(seed, element index), see include/clibd_hip.h."""
    __slots__ = ("seed", "thr16", "scale")

    def __init__(self, p: float, seed: int):
        self.thr16 = int(round(p * 65536.0))
        if not 0 <= self.thr16 < 65536:
            raise ValueError("dropout p must be in [0, 1)")
        self.seed = seed & 0xFFFFFFFF
        self.scale = 1.0 / (1.0 - self.thr16 / 65536.0)


def _drop_args(drop: Optional[Drop]) -> tuple:
    """(seed, thr16, scale) of a dropout site for the C ABI; no site or p = 0: dropout off"""
    return (drop.seed, drop.thr16, drop.scale) if (drop is not None and drop.thr16 > 0) else (0, 0, 1.0)


def derive_seed(base: int, layer: int, site: int) -> int:
    """site seeds of one tower call (site: 0 attention probs, 1 attention-output dropout, 2 output dropout, 3 embeddings)"""
    x = (base ^ ((layer * 8 + site + 1) * 0x9E3779B1)) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


# Measured in-step (profiles/r06_exp_gemm_stream_k_tail.log): 1.8-2.4 % SLOWER at per-GPU batch 256, 0.4-0.7 % slower at 2048 -> off by default (CLIBD_GEMM_STREAMK=1 turns it on)
_STREAMK = os.environ.get("CLIBD_GEMM_STREAMK", "0") == "1"
_TAIL_WS_BYTES = 48 * 1024 * 1024 + 1024

# Every workspace the C ABI takes: uint8 buffers, one per (kind, device, stream), grown on demand.  A workspace is only ever used by launches on
# its own stream, so stream order keeps consecutive users apart.  Kinds: "tail" (stream-K tail of gemm_nt: zero-filled when created, every launch
# leaves it zero), "splitk" (split-K partial tiles, shared by the TN and NT weight-gradient paths), and one per reduction of the deterministic
# mode (the `ordered=True` keyword below).
_workspaces: dict = {"tail": {}}   # kind -> {(device, stream): buffer}
_tail_ws = _workspaces["tail"]


def _workspace(kind: str, nbytes: int, device, zero: bool = False) -> torch.Tensor:
    cache = _workspaces.setdefault(kind, {})
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = (torch.zeros if zero else torch.empty)(((max(int(nbytes), 16) + 15) // 16 * 16,), dtype=torch.uint8, device=device)
        cache[key] = ws
    return ws


def _ws_args(ws: Optional[torch.Tensor]) -> tuple:
    """(workspace, workspace_bytes) of the C ABI; no workspace: (None, 0), the atomic / plain form"""
    return (None, 0) if ws is None else (ws.data_ptr(), ws.numel())


def _not_ordered(what: str):
    """the deterministic mode met a launch that only has an atomic form: an error, never a silent nondeterministic run"""
    from .engine import NotSupportedYet

    return NotSupportedYet(f"deterministic mode: {what} has no fixed-order form")


def gemm_nt(
    a: torch.Tensor,
    w: torch.Tensor,
    *,
    bias: Optional[torch.Tensor] = None,
    rank_u: Optional[torch.Tensor] = None,
    rank_v: Optional[torch.Tensor] = None,
    act: int = ACT_NONE,
    aux: Optional[torch.Tensor] = None,
    residual: Optional[torch.Tensor] = None,
    out_pre: Optional[torch.Tensor] = None,
    out_bf16: Optional[torch.Tensor] = None,
    out_f32: Optional[torch.Tensor] = None,
    split_k: int = 1,
    drop: Optional["Drop"] = None,
    k_hole: Optional[tuple] = None,
    row_sums: Optional[torch.Tensor] = None,
    row_stats: Optional[torch.Tensor] = None,
    col_sum_w: Optional[torch.Tensor] = None,
) -> None:
    """out = epilogue(a[M,K] @ w[N,K]^T); see clibd_gemm_bf16_nt in include/clibd_hip.h.
    k_hole = (k0, length): the K range [k0, k0+length) of both operands is skipped (multiples of 64).
    row_sums (fp32 [N/128, M, 2]) / row_stats (fp32 [M,2]) + col_sum_w (fp32 [N]): the producer / consumer epilogues of the
    LayerNorm -> Linear fold (clibd_gemm_epilogue.row_sums, .row_stats)."""
    _chk(a, BF16, "a", contiguous=False)
    _chk(w, BF16, "w", contiguous=False)
    lda, ldw = _rowmajor(a, "a"), _rowmajor(w, "w")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise ValueError(f"gemm_nt: K mismatch {K} vs {K2}")
    ep = GemmEpilogue()
    ep.act = act
    ep.split_k = split_k
    if drop is not None and drop.thr16 > 0:
        ep.drop_seed, ep.drop_thr16, ep.drop_scale, ep.drop_ld = drop.seed, drop.thr16, drop.scale, N
    if bias is not None:
        _chk(bias, F32, "bias")
        if bias.numel() != N:
            raise ValueError("gemm_nt: bias must have N elements")
        ep.bias = bias.data_ptr()
    if rank_u is not None or rank_v is not None:
        _chk(rank_u, BF16, "rank_u", contiguous=False)
        _chk(rank_v, BF16, "rank_v")
        if rank_u.shape[0] != M or rank_u.shape[1] < 8 or tuple(rank_v.shape) != (N, 8):
            raise ValueError("gemm_nt: rank_u must be [M,>=8], rank_v [N,8]")
        ep.rank_u, ep.rank_v, ep.ld_rank_u = rank_u.data_ptr(), rank_v.data_ptr(), _rowmajor(rank_u, "rank_u")
    if aux is not None:
        _chk(aux, torch.uint8 if act in (ACT_MUL_AUX_U8, ACT_MUL_AUX_E12) else BF16, "aux", contiguous=False)   # _U8: gelu' codes, one byte per element; _E12: 1.5 bytes
        if tuple(aux.shape) != (M, 3 * N // 2 if act == ACT_MUL_AUX_E12 else N):
            raise ValueError("gemm_nt: aux must be [M,N] ([M,3N/2] bytes for the e4m7 form)")
        ep.aux_bf16, ep.ld_aux = aux.data_ptr(), _rowmajor(aux, "aux")
    if residual is not None:
        _chk(residual, F32, "residual", contiguous=False)
        if tuple(residual.shape) != (M, N):
            raise ValueError("gemm_nt: residual must be [M,N]")
        ep.residual_f32, ep.ld_res = residual.data_ptr(), _rowmajor(residual, "residual")
    for name, t, dt in (("out_pre", out_pre, torch.uint8 if act in (ACT_GELU_SAVE_GRAD_U8, ACT_GELU_SAVE_GRAD_E12) else BF16), ("out_bf16", out_bf16, BF16), ("out_f32", out_f32, F32)):
        if t is not None:
            _chk(t, dt, name, contiguous=False)
            if tuple(t.shape) != (M, 3 * N // 2 if (name == "out_pre" and act == ACT_GELU_SAVE_GRAD_E12) else N):
                raise ValueError(f"gemm_nt: {name} must be [M,N] ([M,3N/2] bytes for the e4m7 form)")
    if out_pre is not None:
        ep.out_pre_bf16, ep.ld_pre = out_pre.data_ptr(), _rowmajor(out_pre, "out_pre")
    if out_bf16 is not None:
        ep.out_bf16, ep.ld_out_bf16 = out_bf16.data_ptr(), _rowmajor(out_bf16, "out_bf16")
    if out_f32 is not None:
        ep.out_f32, ep.ld_out_f32 = out_f32.data_ptr(), _rowmajor(out_f32, "out_f32")
    if row_sums is not None:
        _chk(row_sums, F32, "row_sums")
        if N % 128 or tuple(row_sums.shape) != (N // 128, M, 2):
            raise ValueError("gemm_nt: row_sums must be [N/128, M, 2]")
        ep.row_sums = row_sums.data_ptr()
    if row_stats is not None or col_sum_w is not None:
        _chk(row_stats, F32, "row_stats")
        _chk(col_sum_w, F32, "col_sum_w")
        if tuple(row_stats.shape) != (M, 2) or col_sum_w.numel() != N:
            raise ValueError("gemm_nt: row_stats must be [M,2], col_sum_w [N]")
        ep.row_stats, ep.col_sum_w = row_stats.data_ptr(), col_sum_w.data_ptr()
    if k_hole is not None:
        check(_lib.load().clibd_gemm_bf16_nt_khole(a.data_ptr(), lda, w.data_ptr(), ldw, M, N, K, int(k_hole[0]), int(k_hole[1]), C.byref(ep),
                                                   _stream()), "gemm_bf16_nt_khole")
        return
    lib = _lib.load()
    # Stream-K tail (round 6): launches whose last tile round is at most half full and whose contraction is long take a per-(device, stream) workspace
    # (zeroed once; 48 MiB + 1 KiB covers every shape) and cut that round's tiles into K-slices over the idle CUs.  Opt-in: see _STREAMK.
    ws = None
    if _STREAMK and split_k == 1 and M >= 1024:
        need = int(lib.clibd_gemm_tail_workspace_bytes(M, N, K))
        if need > 0:
            ws = _workspace("tail", max(need, _TAIL_WS_BYTES), a.device, zero=True)
    check(lib.clibd_gemm_bf16_nt(a.data_ptr(), lda, w.data_ptr(), ldw, M, N, K, C.byref(ep), *_ws_args(ws), _stream()), "gemm_bf16_nt")


def rowsum_finalize(row_sums: torch.Tensor, eps: float, stats: torch.Tensor) -> None:
    """stats[m] = (mean, rstd) from the fold producer's per-slice sums [S, M, 2] (H = 128 S)."""
    _chk(row_sums, F32, "row_sums")
    _chk(stats, F32, "stats")
    S, M, _ = row_sums.shape
    if tuple(stats.shape) != (M, 2):
        raise ValueError("rowsum_finalize: stats must be [M,2]")
    check(_lib.load().clibd_rowsum_finalize(row_sums.data_ptr(), S, M, 128 * S, float(eps), stats.data_ptr(), _stream()), "rowsum_finalize")


def ln_fold_weights(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor]):
    """(wg bf16 [N,K], col_sum_w fp32 [N], bias_folded fp32 [N]) of a frozen Linear behind LayerNorm(gamma, beta): clibd_ln_fold_weights."""
    _chk(w, F32, "w")
    _chk(gamma, F32, "gamma")
    _chk(beta, F32, "beta")
    N, K = w.shape
    wg = torch.empty((N, K), dtype=BF16, device=w.device)
    s = torch.empty((N,), dtype=F32, device=w.device)
    bp = torch.empty((N,), dtype=F32, device=w.device)
    check(_lib.load().clibd_ln_fold_weights(w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), bias.data_ptr() if bias is not None else None, N, K,
                                            wg.data_ptr(), s.data_ptr(), bp.data_ptr(), _stream()), "ln_fold_weights")
    return wg, s, bp


def quantize_rows_fp8(w: torch.Tensor, act_scale: float):
    """(w_fp8 [N,K] float8_e4m3fn, col_scale [N] fp32) for gemm_fp8_nt; see clibd_quantize_rows_fp8."""
    _chk(w, F32, "w")
    N, K = w.shape
    w8 = torch.empty((N, K), dtype=torch.uint8, device=w.device).view(FP8)
    cs = torch.empty((N,), dtype=F32, device=w.device)
    check(_lib.load().clibd_quantize_rows_fp8(w.data_ptr(), N, K, float(act_scale), w8.data_ptr(), cs.data_ptr(), _stream()), "quantize_rows_fp8")
    return w8, cs


def quantize_rows_fp8_bf16(w: torch.Tensor, act_scale: float = 1.0, l1max: Optional[torch.Tensor] = None):
    """(w_fp8 [N,K] float8_e4m3fn, col_scale [N] fp32) from a bf16 matrix (a transposed weight shadow): the W operand of gemm_fp8_dgrad_nt.
    l1max (fp32 scalar tensor, zeroed by the caller): raised to the largest row l1 norm of the de-quantised image."""
    _chk(w, BF16, "w")
    N, K = w.shape
    w8 = torch.empty((N, K), dtype=torch.uint8, device=w.device).view(FP8)
    cs = torch.empty((N,), dtype=F32, device=w.device)
    if l1max is not None:
        _chk(l1max, F32, "l1max")
    check(_lib.load().clibd_quantize_rows_fp8_bf16(w.data_ptr(), N, K, float(act_scale), w8.data_ptr(), cs.data_ptr(), _p(l1max), _stream()),
          "quantize_rows_fp8_bf16")
    return w8, cs


def gemm_fp8_dgrad_nt(a: torch.Tensor, w: torch.Tensor, col_scale: torch.Tensor, *, a_row_dequant: Optional[torch.Tensor] = None,
                      aux: Optional[torch.Tensor] = None, act: int = ACT_NONE, out_bf16: Optional[torch.Tensor] = None,
                      out_fp8: Optional[torch.Tensor] = None, out_fp8_scale: float = 0.0, out_bf16_dual: Optional[torch.Tensor] = None) -> None:
    """8-bit dgrad (clibd_gemm_fp8_dgrad_nt): a [M,K] e4m3 gradient rows with per-row scales (a_row_dequant [M] = 1 / scale), w [N,K] the
    transposed weight from quantize_rows_fp8_bf16.  Forms: act NONE -> out_bf16 | ACT_ADD_AUX + aux -> out_bf16 (both need a_row_dequant) |
    ACT_MUL_AUX (bf16 aux) / ACT_MUL_AUX_U8 (one-byte gelu' codes) -> out_fp8 = e4m3(value * out_fp8_scale), which keeps a's row scales;
    out_bf16_dual (full fine-tune; MUL_AUX forms, needs a_row_dequant): also the de-scaled value as bf16, the weight gradient's operand."""
    _chk(a, FP8, "a", contiguous=False)
    _chk(w, FP8, "w", contiguous=False)
    _chk(col_scale, F32, "col_scale")
    lda, ldw = _rowmajor(a, "a"), _rowmajor(w, "w")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2 or col_scale.numel() != N:
        raise ValueError("gemm_fp8_dgrad_nt: shape mismatch")
    if act not in (ACT_NONE, ACT_ADD_AUX, ACT_MUL_AUX, ACT_MUL_AUX_U8, ACT_MUL_AUX_E12):
        raise ValueError("gemm_fp8_dgrad_nt: act must be NONE, ADD_AUX, MUL_AUX, MUL_AUX_U8 or MUL_AUX_E12")
    if (act == ACT_NONE) != (aux is None):
        raise ValueError("gemm_fp8_dgrad_nt: aux comes with ADD_AUX / MUL_AUX only")
    ep = GemmEpilogue()
    ep.split_k = 1
    ep.act = act
    if aux is not None:
        _chk(aux, torch.uint8 if act in (ACT_MUL_AUX_U8, ACT_MUL_AUX_E12) else BF16, "aux", contiguous=False)
        if tuple(aux.shape) != (M, 3 * N // 2 if act == ACT_MUL_AUX_E12 else N):
            raise ValueError("gemm_fp8_dgrad_nt: aux must be [M,N] ([M,3N/2] bytes for the e4m7 form)")
        ep.aux_bf16, ep.ld_aux = aux.data_ptr(), _rowmajor(aux, "aux")
    if act in (ACT_MUL_AUX, ACT_MUL_AUX_U8, ACT_MUL_AUX_E12):
        if out_fp8 is None or out_bf16 is not None or not out_fp8_scale > 0:
            raise ValueError("gemm_fp8_dgrad_nt: the MUL_AUX form writes out_fp8 with a positive out_fp8_scale")
        _chk(out_fp8, FP8, "out_fp8", contiguous=False)
        if tuple(out_fp8.shape) != (M, N):
            raise ValueError("gemm_fp8_dgrad_nt: out_fp8 must be [M,N]")
        ep.out_bf16, ep.ld_out_bf16 = out_fp8.data_ptr(), _rowmajor(out_fp8, "out_fp8")
        if out_bf16_dual is not None:
            if a_row_dequant is None:
                raise ValueError("gemm_fp8_dgrad_nt: out_bf16_dual needs a_row_dequant")
            _chk(out_bf16_dual, BF16, "out_bf16_dual", contiguous=False)
            if tuple(out_bf16_dual.shape) != (M, N):
                raise ValueError("gemm_fp8_dgrad_nt: out_bf16_dual must be [M,N]")
            ep.out_pre_bf16, ep.ld_pre = out_bf16_dual.data_ptr(), _rowmajor(out_bf16_dual, "out_bf16_dual")
    else:
        if out_bf16_dual is not None:
            raise ValueError("gemm_fp8_dgrad_nt: out_bf16_dual comes with the MUL_AUX forms only")
        if out_bf16 is None or out_fp8 is not None or a_row_dequant is None:
            raise ValueError("gemm_fp8_dgrad_nt: the bf16-output forms need out_bf16 and a_row_dequant")
        _chk(out_bf16, BF16, "out_bf16", contiguous=False)
        if tuple(out_bf16.shape) != (M, N):
            raise ValueError("gemm_fp8_dgrad_nt: out_bf16 must be [M,N]")
        ep.out_bf16, ep.ld_out_bf16 = out_bf16.data_ptr(), _rowmajor(out_bf16, "out_bf16")
        out_fp8_scale = 0.0
    if a_row_dequant is not None:
        _chk(a_row_dequant, F32, "a_row_dequant")
        if a_row_dequant.numel() != M:
            raise ValueError("gemm_fp8_dgrad_nt: a_row_dequant must have M elements")
    check(_lib.load().clibd_gemm_fp8_dgrad_nt(a.data_ptr(), lda, w.data_ptr(), ldw, M, N, K, col_scale.data_ptr(), _p(a_row_dequant),
                                              float(out_fp8_scale), C.byref(ep), _stream()), "gemm_fp8_dgrad_nt")


def gemm_fp8_nt(
    a: torch.Tensor,
    w: torch.Tensor,
    col_scale: torch.Tensor,
    *,
    bias: torch.Tensor,
    rank_u: Optional[torch.Tensor] = None,
    rank_v: Optional[torch.Tensor] = None,
    gelu_out_fp8: Optional[torch.Tensor] = None,
    gelu_out_scale: float = 0.0,
    out_pre: Optional[torch.Tensor] = None,
    residual: Optional[torch.Tensor] = None,
    out_bf16: Optional[torch.Tensor] = None,
    out_f32: Optional[torch.Tensor] = None,
    drop: Optional["Drop"] = None,
) -> None:
    """fp8-forward GEMM: epilogue((a[M,K] @ w[N,K]^T) * col_scale[n]) with OCP e4m3 operands; see clibd_gemm_fp8_nt.
    Forms: -> out_bf16 (optionally + rank update) | gelu -> gelu_out_fp8 (= fp8(gelu * gelu_out_scale)) + out_pre (gelu') |
    [dropout] + residual -> out_f32."""
    _chk(a, FP8, "a", contiguous=False)
    _chk(w, FP8, "w", contiguous=False)
    _chk(col_scale, F32, "col_scale")
    _chk(bias, F32, "bias")
    lda, ldw = _rowmajor(a, "a"), _rowmajor(w, "w")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2 or col_scale.numel() != N or bias.numel() != N:
        raise ValueError("gemm_fp8_nt: shape mismatch")
    ep = GemmEpilogue()
    ep.split_k = 1
    ep.bias = bias.data_ptr()
    if drop is not None and drop.thr16 > 0:
        ep.drop_seed, ep.drop_thr16, ep.drop_scale, ep.drop_ld = drop.seed, drop.thr16, drop.scale, N
    if rank_u is not None or rank_v is not None:
        _chk(rank_u, BF16, "rank_u", contiguous=False)
        _chk(rank_v, BF16, "rank_v")
        if rank_u.shape[0] != M or rank_u.shape[1] < 8 or tuple(rank_v.shape) != (N, 8):
            raise ValueError("gemm_fp8_nt: rank_u must be [M,>=8], rank_v [N,8]")
        ep.rank_u, ep.rank_v, ep.ld_rank_u = rank_u.data_ptr(), rank_v.data_ptr(), _rowmajor(rank_u, "rank_u")
    for name, t, dt in (("out_pre", out_pre, BF16), ("out_bf16", out_bf16, BF16), ("out_f32", out_f32, F32), ("residual", residual, F32),
                        ("gelu_out_fp8", gelu_out_fp8, FP8)):
        if t is not None:
            _chk(t, dt, name, contiguous=False)
            if tuple(t.shape) != (M, N):
                raise ValueError(f"gemm_fp8_nt: {name} must be [M,N]")
    out_scale = 0.0
    if gelu_out_fp8 is not None:
        if out_pre is None or out_bf16 is not None or gelu_out_scale <= 0:
            raise ValueError("gemm_fp8_nt: the gelu form needs out_pre and a positive gelu_out_scale, and no out_bf16")
        ep.act = ACT_GELU_SAVE_GRAD
        ep.out_pre_bf16, ep.ld_pre = out_pre.data_ptr(), _rowmajor(out_pre, "out_pre")
        ep.out_bf16, ep.ld_out_bf16 = gelu_out_fp8.data_ptr(), _rowmajor(gelu_out_fp8, "gelu_out_fp8")
        out_scale = float(gelu_out_scale)
    elif out_bf16 is not None:
        ep.out_bf16, ep.ld_out_bf16 = out_bf16.data_ptr(), _rowmajor(out_bf16, "out_bf16")
    if residual is not None:
        ep.residual_f32, ep.ld_res = residual.data_ptr(), _rowmajor(residual, "residual")
    if out_f32 is not None:
        ep.out_f32, ep.ld_out_f32 = out_f32.data_ptr(), _rowmajor(out_f32, "out_f32")
    check(_lib.load().clibd_gemm_fp8_nt(a.data_ptr(), lda, w.data_ptr(), ldw, M, N, K, col_scale.data_ptr(), out_scale, C.byref(ep), _stream()),
          "gemm_fp8_nt")


def transpose_bf16(x: torch.Tensor, pad_to: int = 64, colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R,C] bf16 -> [C, R_pad] bf16 (zero padded along R to a multiple of `pad_to`).
    colsum (fp32 [C], accumulates): column sums of x in the same pass (bias gradient beside the weight gradient's dy^T), through a
    partials workspace and a fixed-order second kernel (always: no float atomics, bit-reproducible)."""
    _chk(x, BF16, "x", contiguous=False)
    ld = _rowmajor(x, "x")
    R, Cc = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    out = torch.empty((Cc, Rp), dtype=BF16, device=x.device)
    if colsum is not None:
        _chk(colsum, F32, "colsum")
        if colsum.numel() != Cc:
            raise ValueError("transpose_bf16: colsum must have C elements")
        lib = _lib.load()
        need = int(lib.clibd_transpose_colsum_workspace_bytes(Rp, Cc))
        ws = torch.empty(((need + 3) // 4,), dtype=F32, device=x.device)
        check(lib.clibd_transpose_colsum_bf16(x.data_ptr(), ld, R, Cc, out.data_ptr(), Rp, colsum.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream()),
              "transpose_colsum_bf16")
    else:
        check(_lib.load().clibd_transpose_bf16(x.data_ptr(), ld, R, Cc, out.data_ptr(), Rp, _stream()), "transpose_bf16")
    return out


def transpose_fp8(x: torch.Tensor, scale: float, pad_to: int = 64) -> torch.Tensor:
    """[R,C] float8_e4m3fn -> [C, R_pad] bf16 holding x * scale (zero padded along R to a multiple of `pad_to`): the transposed,
    dequantised X operand of a weight gradient under the fp8 forward (scale = 1 / the quantisation scale; a power of two is exact)."""
    _chk(x, FP8, "x", contiguous=False)
    ld = _rowmajor(x, "x")
    R, Cc = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    out = torch.empty((Cc, Rp), dtype=BF16, device=x.device)
    check(_lib.load().clibd_transpose_fp8_bf16(x.data_ptr(), ld, R, Cc, float(scale), out.data_ptr(), Rp, _stream()), "transpose_fp8_bf16")
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    _chk(x, F32, "x")
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(_lib.load().clibd_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "cast_f32_to_bf16")
    return out


def cast_transpose_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 [R,C] -> bf16 [C,R]."""
    _chk(x, F32, "x")
    R, Cc = x.shape
    out = torch.empty((Cc, R), dtype=BF16, device=x.device)
    check(_lib.load().clibd_cast_transpose_f32_to_bf16(x.data_ptr(), R, Cc, out.data_ptr(), _stream()), "cast_transpose")
    return out


def layernorm_fwd(x, gamma, beta, eps, *, y_bf16=None, y_f32=None, stats=None, lora_a=None, t_out=None, drop=None,
                  y_fp8=None, fp8_scale: float = 0.0) -> None:
    """y_fp8 (fp8-forward mode): also / only emit e4m3(y * fp8_scale), the operand of the next gemm_fp8_nt."""
    _chk(x, F32, "x")
    M, H = x.shape
    _chk(gamma, F32, "gamma")
    _chk(beta, F32, "beta")
    for nm, t, dt, shape in (("y_bf16", y_bf16, BF16, (M, H)), ("y_f32", y_f32, F32, (M, H)), ("stats", stats, F32, (M, 2)),
                             ("lora_a", lora_a, BF16, (8, H)), ("t_out", t_out, BF16, (M, 8)), ("y_fp8", y_fp8, FP8, (M, H))):
        if t is not None:
            _chk(t, dt, nm)
            if tuple(t.shape) != shape:
                raise ValueError(f"layernorm_fwd: {nm} must be {shape}, got {tuple(t.shape)}")
    check(_lib.load().clibd_layernorm_fwd(x.data_ptr(), M, H, gamma.data_ptr(), beta.data_ptr(), float(eps), _p(y_bf16), _p(y_f32),
                                          _p(stats), _p(lora_a), _p(t_out), *_drop_args(drop), _p(y_fp8), float(fp8_scale), _stream()),
          "layernorm_fwd")


def layernorm_bwd(dy, x, stats, gamma, *, dres=None, dx_f32=None, dx_bf16=None, drop=None, dgamma=None, dbeta=None,
                  dres_bf16=None, dx_res_bf16=None, dx_fp8=None, row_dequant=None, ordered: bool = False) -> None:
    """dx = LN'(dy) [+ dres | dres_bf16] into dx_f32 / dx_bf16 / dx_res_bf16 (at least one); see clibd_layernorm_bwd in include/clibd_hip.h.
    dgamma / dbeta (fp32 [H], accumulate): the LayerNorm parameter gradients in the same pass (full fine-tune mode).
    dres_bf16 / dx_res_bf16: the residual gradient travels as bf16: dx = LN'(dy) + dres_bf16, dx_res_bf16 = bf16(dx) without the
    dropout mask that dx_bf16 carries.
    dx_fp8 [M,H] e4m3 + row_dequant [M] fp32 (8-bit dgrad): the dx_bf16 values once more as the A operand of gemm_fp8_dgrad_nt, one
    power-of-two scale per row; dx_bf16 itself becomes optional.
    ordered (with dgamma / dbeta): the parameter gradients as per-block partials summed in block order."""
    _chk(x, F32, "x")
    M, H = x.shape
    if dy.dtype not in (BF16, F32):
        raise ValueError("layernorm_bwd: dy must be bf16 or fp32")
    _chk(stats, F32, "stats")
    _chk(gamma, F32, "gamma")
    for nm, t, dt, shape in (("dy", dy, dy.dtype, (M, H)), ("dres", dres, F32, (M, H)), ("dres_bf16", dres_bf16, BF16, (M, H)),
                             ("dx_f32", dx_f32, F32, (M, H)), ("dx_res_bf16", dx_res_bf16, BF16, (M, H)), ("dx_bf16", dx_bf16, BF16, (M, H)),
                             ("dx_fp8", dx_fp8, FP8, (M, H)), ("row_dequant", row_dequant, F32, (M,)), ("dgamma", dgamma, F32, (H,)),
                             ("dbeta", dbeta, F32, (H,))):
        if t is not None:
            _chk(t, dt, nm)
            if tuple(t.shape) != shape and (len(shape) == 2 or t.numel() != shape[0]):   # the vectors: any shape of that many elements
                raise ValueError(f"layernorm_bwd: {nm} must be {shape}, got {tuple(t.shape)}")
    if (dx_fp8 is None) != (row_dequant is None) or (dgamma is None) != (dbeta is None):
        raise ValueError("layernorm_bwd: dx_fp8 comes with row_dequant, dgamma with dbeta")
    if dres is not None and dres_bf16 is not None:
        raise ValueError("layernorm_bwd: the residual gradient is either fp32 (dres) or bf16 (dres_bf16)")
    if dx_f32 is None and dx_bf16 is None and dx_res_bf16 is None and dx_fp8 is None:
        raise ValueError("layernorm_bwd: no output")
    lib = _lib.load()
    ws = _workspace("ln_pg", int(lib.clibd_layernorm_bwd_pg_workspace_bytes(M, H)), x.device) if ordered and dgamma is not None else None
    dyb, dyf = (dy.data_ptr(), None) if dy.dtype == BF16 else (None, dy.data_ptr())
    check(lib.clibd_layernorm_bwd(dyb, dyf, x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), M, H, _p(dres), _p(dres_bf16), _p(dx_f32),
                                  _p(dx_res_bf16), _p(dx_bf16), *_drop_args(drop), _p(dx_fp8), _p(row_dequant), _p(dgamma), _p(dbeta),
                                  *_ws_args(ws), _stream()), "layernorm_bwd")


def attention_fwd(qkv: torch.Tensor, B: int, S: int, nheads: int, key_mask: Optional[torch.Tensor], out: torch.Tensor,
                  nq: Optional[int] = None, drop=None, out_fp8_scale: float = 0.0, lse: Optional[torch.Tensor] = None,
                  o_lo: Optional[torch.Tensor] = None) -> None:
    """nq: evaluate only the first nq query rows of every sequence; `out` is then [B*nq, H].
    out_fp8_scale > 0 (fp8-forward mode): `out` is float8_e4m3fn and receives e4m3(o * out_fp8_scale).
    lse (fp32 [B*nheads*S]) + o_lo (bf16 [B*S, H]): the saving forward, for attention_bwd_sp."""
    _chk(qkv, BF16, "qkv")
    H = nheads * 64
    nq = S if nq is None else nq
    if lse is not None or o_lo is not None:
        _chk(lse, F32, "lse"); _chk(o_lo, BF16, "o_lo")
        if nq != S or out_fp8_scale > 0 or tuple(o_lo.shape) != (B * S, H) or lse.numel() != B * nheads * S:
            raise ValueError("attention_fwd: the saving form needs nq = S, bf16 out [B*S,H], o_lo [B*S,H], lse [B*nheads*S]")
    _chk(out, FP8 if out_fp8_scale > 0 else BF16, "out")
    if tuple(qkv.shape) != (B * S, 3 * H) or tuple(out.shape) != (B * nq, H):
        raise ValueError("attention_fwd: qkv must be [B*S,3H], out [B*nq,H] with H = 64*nheads")
    if key_mask is not None:
        _chk(key_mask, I32, "key_mask")
        if tuple(key_mask.shape) != (B, S):
            raise ValueError("attention_fwd: key_mask must be [B,S]")
    check(_lib.load().clibd_attention_fwd(qkv.data_ptr(), B, S, nheads, _p(key_mask), out.data_ptr(), nq, nq, *_drop_args(drop),
                                          float(out_fp8_scale), _p(lse), _p(o_lo), _stream()), "attention_fwd")


def attention_bwd(qkv, dout, B, S, nheads, key_mask, dqkv, nq: Optional[int] = None, drop=None) -> None:
    """nq: `dout` is [B*nq, H] — the gradient of the first nq query rows of every sequence (the rest is zero)."""
    _chk(qkv, BF16, "qkv")
    _chk(dout, BF16, "dout")
    _chk(dqkv, BF16, "dqkv")
    H = nheads * 64
    nq = S if nq is None else nq
    if tuple(qkv.shape) != (B * S, 3 * H) or tuple(dout.shape) != (B * nq, H) or tuple(dqkv.shape) != (B * S, 3 * H):
        raise ValueError("attention_bwd: shapes")
    if key_mask is not None:
        _chk(key_mask, I32, "key_mask")
    check(_lib.load().clibd_attention_bwd(qkv.data_ptr(), dout.data_ptr(), B, S, nheads, _p(key_mask), dqkv.data_ptr(), nq, nq,
                                          *_drop_args(drop), _stream()), "attention_bwd")


def attention_bwd_sp(qkv, dout, out, o_lo, lse, B, S, nheads, dqkv, drop=None) -> None:
    """Single-pass backward from the forward's saved output, rounding residual and log-sum-exp (clibd_attention_bwd_sp):
    full sequences, no key mask, S <= 224."""
    H = nheads * 64
    for nm, t, shape in (("qkv", qkv, (B * S, 3 * H)), ("dout", dout, (B * S, H)), ("out", out, (B * S, H)), ("o_lo", o_lo, (B * S, H)),
                         ("dqkv", dqkv, (B * S, 3 * H))):
        _chk(t, BF16, nm)
        if tuple(t.shape) != shape:
            raise ValueError(f"attention_bwd_sp: {nm} must be {shape}")
    _chk(lse, F32, "lse")
    if lse.numel() != B * nheads * S:
        raise ValueError("attention_bwd_sp: lse must have B*nheads*S elements")
    check(_lib.load().clibd_attention_bwd_sp(qkv.data_ptr(), dout.data_ptr(), out.data_ptr(), o_lo.data_ptr(), lse.data_ptr(), B, S, nheads,
                                             dqkv.data_ptr(), *_drop_args(drop), _stream()), "attention_bwd_sp")


def _wide_shapes(op: str, B: int, S: int, nheads: int, head_dim: int, named) -> None:
    H = nheads * head_dim
    for nm, t, cols in named:
        _chk(t, BF16, nm)
        if tuple(t.shape) != (B * S, cols * H):
            raise ValueError(f"{op}: {nm} must be [B*S, {cols}H] with H = nheads*head_dim = {H}")


def attention_wide_fwd(qkv: torch.Tensor, B: int, S: int, nheads: int, head_dim: int, out: torch.Tensor, lse: Optional[torch.Tensor] = None,
                       drop=None) -> None:
    """Attention for 128- / 192-wide heads (clibd_attention_wide_fwd): full sequences, no key mask, bf16 out [B*S, H].
    lse (fp32 [B*nheads*S], optional): the log2-domain log-sum-exp attention_wide_bwd needs."""
    _wide_shapes("attention_wide_fwd", B, S, nheads, head_dim, (("qkv", qkv, 3), ("out", out, 1)))
    if lse is not None:
        _chk(lse, F32, "lse")
        if lse.numel() != B * nheads * S:
            raise ValueError("attention_wide_fwd: lse must have B*nheads*S elements")
    check(_lib.load().clibd_attention_wide_fwd(qkv.data_ptr(), B, S, nheads, head_dim, out.data_ptr(), _p(lse), *_drop_args(drop), _stream()),
          "attention_wide_fwd")


def attention_wide_bwd(qkv, dout, lse, B: int, S: int, nheads: int, head_dim: int, dqkv, drop=None) -> None:
    """dqkv [B*S, 3H] (every row, all three sections) from qkv, dout [B*S, H] and the forward's lse (clibd_attention_wide_bwd)."""
    _wide_shapes("attention_wide_bwd", B, S, nheads, head_dim, (("qkv", qkv, 3), ("dout", dout, 1), ("dqkv", dqkv, 3)))
    if lse is None:
        raise ValueError("attention_wide_bwd: needs the lse the forward wrote")
    _chk(lse, F32, "lse")
    if lse.numel() != B * nheads * S:
        raise ValueError("attention_wide_bwd: lse must have B*nheads*S elements")
    check(_lib.load().clibd_attention_wide_bwd(qkv.data_ptr(), dout.data_ptr(), lse.data_ptr(), B, S, nheads, head_dim, dqkv.data_ptr(),
                                               *_drop_args(drop), _stream()), "attention_wide_bwd")


def lora_pack(a_q, a_v, b_q, b_v, v_fwd, v_bwd, a_cat, w_dt) -> None:
    H = a_q.shape[1]
    for nm, t, shape in (("a_q", a_q, (4, H)), ("a_v", a_v, (4, H)), ("b_q", b_q, (H, 4)), ("b_v", b_v, (H, 4))):
        _chk(t, F32, nm)
        if tuple(t.shape) != shape:
            raise ValueError(f"lora_pack: {nm} must be {shape}")
    for nm, t, shape in (("v_fwd", v_fwd, (3 * H, 8)), ("v_bwd", v_bwd, (H, 8)), ("a_cat", a_cat, (8, H)), ("w_dt", w_dt, (16, 3 * H))):
        _chk(t, BF16, nm)
        if tuple(t.shape) != shape:
            raise ValueError(f"lora_pack: {nm} must be {shape}")
    check(_lib.load().clibd_lora_pack(a_q.data_ptr(), a_v.data_ptr(), b_q.data_ptr(), b_v.data_ptr(), H, v_fwd.data_ptr(),
                                      v_bwd.data_ptr(), a_cat.data_ptr(), w_dt.data_ptr(), _stream()), "lora_pack")


def lora_down_proj(x: torch.Tensor, a_cat: torch.Tensor) -> torch.Tensor:
    """t [M,8] = bf16(x [M,H] . a_cat [8,H]^T): the adapters' down-projection as its own kernel (rank slots after the first, r > 4)."""
    _chk(x, BF16, "x", contiguous=False)
    _chk(a_cat, BF16, "a_cat")
    M, H = x.shape
    if tuple(a_cat.shape) != (8, H):
        raise ValueError("lora_down_proj: a_cat must be [8,H]")
    t = torch.empty((M, 8), dtype=BF16, device=x.device)
    check(_lib.load().clibd_lora_down_proj(x.data_ptr(), _rowmajor(x, "x"), a_cat.data_ptr(), M, H, t.data_ptr(), _stream()), "lora_down_proj")
    return t


def _lora_workspace(M: int, H: int, device, workspace):
    """(pointer, bytes) of the adapters' partials workspace: the caller's buffer, a fresh one (deterministic sums, no contended
    float atomics), or (None, 0) when `workspace` is False (the float atomics of rounds 1-4) / the shape takes the VALU kernel."""
    if workspace is False:
        return None, 0
    need = int(_lib.load().clibd_lora_workspace_bytes(M, H))
    if need == 0:
        return None, 0
    if workspace is None or workspace is True:
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError("lora workspace too small (clibd_lora_workspace_bytes)")
    return workspace, need


def lora_wgrad(dqkv, x, t, dt, dA_q, dA_v, dB_q, dB_v, workspace=None) -> None:
    _chk(dqkv, BF16, "dqkv")
    _chk(x, BF16, "x")
    _chk(t, BF16, "t")
    _chk(dt, BF16, "dt")
    M, H = x.shape
    if tuple(dqkv.shape) != (M, 3 * H) or tuple(t.shape) != (M, 8) or dt.shape[0] != M or dt.shape[1] < 8:
        raise ValueError("lora_wgrad: shapes")
    for nm, g, shape in (("dA_q", dA_q, (4, H)), ("dA_v", dA_v, (4, H)), ("dB_q", dB_q, (H, 4)), ("dB_v", dB_v, (H, 4))):
        _chk(g, F32, nm)
        if tuple(g.shape) != shape:
            raise ValueError(f"lora_wgrad: {nm} must be {shape}")
    ws, nb = _lora_workspace(M, H, x.device, workspace)
    check(_lib.load().clibd_lora_wgrad(dqkv.data_ptr(), 3 * H, x.data_ptr(), t.data_ptr(), dt.data_ptr(), dt.shape[1], M, H,
                                       dA_q.data_ptr(), dA_v.data_ptr(), dB_q.data_ptr(), dB_v.data_ptr(),
                                       ws.data_ptr() if ws is not None else None, nb, _stream()), "lora_wgrad")


def lora_backward(dqkv, x, t, w_dt, dt, dA_q, dA_v, dB_q, dB_v, workspace=None, ordered: bool = False) -> None:
    """dt = dqkv . w_dt^T (written, bf16 [M,16]) and the adapters' four parameter gradients (accumulated); see clibd_lora_backward.
    workspace: None = a partials buffer is allocated (deterministic, atomics-free sums), a uint8 tensor = the caller's, False = float atomics.
    ordered: a token count that is not a multiple of 32 (which would take the VALU kernel and its float atomics) runs as whole 32-row slabs,
    zero-padded — the padded rows contribute exact zeros to every sum; whole-slab counts run exactly as without it."""
    _chk(dqkv, BF16, "dqkv")
    _chk(x, BF16, "x")
    _chk(t, BF16, "t")
    _chk(w_dt, BF16, "w_dt")
    _chk(dt, BF16, "dt")
    M, H = x.shape
    if tuple(dqkv.shape) != (M, 3 * H) or tuple(t.shape) != (M, 8) or tuple(w_dt.shape) != (16, 3 * H) or tuple(dt.shape) != (M, 16):
        raise ValueError("lora_backward: shapes")
    for nm, g, shape in (("dA_q", dA_q, (4, H)), ("dA_v", dA_v, (4, H)), ("dB_q", dB_q, (H, 4)), ("dB_v", dB_v, (H, 4))):
        _chk(g, F32, nm)
        if tuple(g.shape) != shape:
            raise ValueError(f"lora_backward: {nm} must be {shape}")
    if ordered:
        if workspace is False:
            raise _not_ordered("lora_backward without a workspace")
        if M % 32:
            Mp = (M + 31) // 32 * 32
            pad = lambda a: torch.cat([a, a.new_zeros((Mp - M, a.shape[1]))], dim=0)
            dtp = torch.empty((Mp, 16), dtype=BF16, device=dt.device)
            lora_backward(pad(dqkv), pad(x), pad(t), w_dt, dtp, dA_q, dA_v, dB_q, dB_v, workspace=None, ordered=True)
            dt.copy_(dtp[:M])
            return
        if int(_lib.load().clibd_lora_workspace_bytes(M, H)) == 0:
            raise _not_ordered(f"lora_backward at M={M}, H={H}")
    ws, nb = _lora_workspace(M, H, x.device, workspace)
    check(_lib.load().clibd_lora_backward(dqkv.data_ptr(), 3 * H, x.data_ptr(), t.data_ptr(), w_dt.data_ptr(), dt.data_ptr(), 16, M, H,
                                          dA_q.data_ptr(), dA_v.data_ptr(), dB_q.data_ptr(), dB_v.data_ptr(),
                                          ws.data_ptr() if ws is not None else None, nb, _stream()), "lora_backward")


def patchify(image: torch.Tensor) -> torch.Tensor:
    """fp32 [B,3,224,224] in [0,1] — or the dataset's uint8 bytes, read as u8 / 255 (bit-identical to the fp32 form of the same
    image: clibd_patchify_u8) — -> bf16 patch matrix [B*196, 768]."""
    _chk(image, torch.uint8 if image.dtype == torch.uint8 else F32, "image")
    if image.dim() != 4 or tuple(image.shape[1:]) != (3, 224, 224):
        raise ValueError("patchify: image must be [B,3,224,224]")
    B = image.shape[0]
    out = torch.empty((B * 196, 768), dtype=BF16, device=image.device)
    if image.dtype == torch.uint8:
        check(_lib.load().clibd_patchify_u8(image.data_ptr(), B, out.data_ptr(), _stream()), "patchify_u8")
    else:
        check(_lib.load().clibd_patchify(image.data_ptr(), B, out.data_ptr(), _stream()), "patchify")
    return out


def vit_assemble_tokens(proj: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, B: int) -> torch.Tensor:
    """tok[b,0] = cls + pos[0]; tok[b,1+p] = proj[b*P+p] + pos[1+p]  -> fp32 [B,S,H]"""
    _chk(proj, F32, "proj")
    _chk(cls, F32, "cls")
    _chk(pos, F32, "pos")
    H = proj.shape[1]
    S = pos.numel() // H
    if proj.shape[0] != B * (S - 1) or cls.numel() != H:
        raise ValueError("vit_assemble_tokens: shapes")
    tok = torch.empty((B, S, H), dtype=F32, device=proj.device)
    check(_lib.load().clibd_vit_assemble_tokens(proj.data_ptr(), cls.data_ptr(), pos.data_ptr(), B, S, H, tok.data_ptr(), _stream()),
          "vit_assemble_tokens")
    return tok


def gelu_bwd(dy: torch.Tensor, pre: torch.Tensor) -> torch.Tensor:
    _chk(dy, BF16, "dy")
    _chk(pre, BF16, "pre")
    if dy.shape != pre.shape:
        raise ValueError("gelu_bwd: shapes")
    dx = torch.empty_like(dy)
    check(_lib.load().clibd_gelu_bwd_bf16(dy.data_ptr(), pre.data_ptr(), dy.numel(), dx.data_ptr(), _stream()), "gelu_bwd")
    return dx


def bert_embed(ids, token_type, word, pos, typ, out) -> None:
    _chk(ids, I64, "ids")
    B, S = ids.shape
    H = word.shape[1]
    if token_type is not None:
        _chk(token_type, I64, "token_type")
    for nm, t in (("word", word), ("pos", pos), ("type", typ), ("out", out)):
        _chk(t, F32, nm)
    if pos.shape[0] < S:
        raise ValueError("bert_embed: sequence longer than the position table")
    check(_lib.load().clibd_bert_embed(ids.data_ptr(), _p(token_type), B, S, H, word.shape[0], word.data_ptr(), pos.data_ptr(),
                                       typ.data_ptr(), out.data_ptr(), _stream()), "bert_embed")


def softmax_mean_fwd(logits: torch.Tensor, B: int, S: int) -> torch.Tensor:
    _chk(logits, BF16, "logits")
    Cc = logits.shape[1]
    out = torch.empty((B, Cc), dtype=F32, device=logits.device)
    check(_lib.load().clibd_softmax_mean_fwd(logits.data_ptr(), B, S, Cc, out.data_ptr(), _stream()), "softmax_mean_fwd")
    return out


def softmax_mean_bwd(logits: torch.Tensor, dout: torch.Tensor, B: int, S: int) -> torch.Tensor:
    _chk(logits, BF16, "logits")
    _chk(dout, F32, "dout")
    Cc = logits.shape[1]
    dl = torch.empty_like(logits)
    check(_lib.load().clibd_softmax_mean_bwd(logits.data_ptr(), dout.data_ptr(), B, S, Cc, dl.data_ptr(), _stream()), "softmax_mean_bwd")
    return dl


def token_mean_fwd(x: torch.Tensor) -> torch.Tensor:
    _chk(x, F32, "x")
    B, S, H = x.shape
    out = torch.empty((B, H), dtype=BF16, device=x.device)
    check(_lib.load().clibd_token_mean_fwd(x.data_ptr(), B, S, H, out.data_ptr(), _stream()), "token_mean_fwd")
    return out


def token_mean_bwd(dout: torch.Tensor, S: int) -> torch.Tensor:
    _chk(dout, F32, "dout")
    B, H = dout.shape
    dx = torch.empty((B, S, H), dtype=F32, device=dout.device)
    check(_lib.load().clibd_token_mean_bwd(dout.data_ptr(), B, S, H, dx.data_ptr(), _stream()), "token_mean_bwd")
    return dx


def colsum_bf16(x: torch.Tensor, out: torch.Tensor, ordered: bool = False) -> None:
    """out[N] (fp32) += column sums of x[M,N] (bf16).  ordered: per-chunk partials summed in chunk order."""
    _chk(x, BF16, "x", contiguous=False)
    _chk(out, F32, "out")
    M, N = x.shape
    lib = _lib.load()
    ws = _workspace("colsum", int(lib.clibd_colsum_workspace_bytes(M, N)), x.device) if ordered else None
    check(lib.clibd_colsum_bf16(x.data_ptr(), _rowmajor(x, "x"), M, N, out.data_ptr(), *_ws_args(ws), _stream()), "colsum_bf16")


def gather_rows(x: torch.Tensor) -> torch.Tensor:
    _chk(x, F32, "x")
    B, S, H = x.shape
    out = torch.empty((B, H), dtype=F32, device=x.device)
    check(_lib.load().clibd_gather_rows(x.data_ptr(), B, S, H, out.data_ptr(), _stream()), "gather_rows")
    return out


def scatter_rows(dcls: torch.Tensor, S: int, *, bf16: bool = True, f32: bool = False):
    _chk(dcls, F32, "dcls")
    B, H = dcls.shape
    ob = torch.empty((B * S, H), dtype=BF16, device=dcls.device) if bf16 else None
    of = torch.empty((B * S, H), dtype=F32, device=dcls.device) if f32 else None
    check(_lib.load().clibd_scatter_rows_bf16(dcls.data_ptr(), B, S, H, _p(ob), _p(of), _stream()), "scatter_rows")
    return ob, of


def l2norm_fwd(x: torch.Tensor):
    _chk(x, F32, "x")
    N, D = x.shape
    y = torch.empty_like(x)
    inv = torch.empty((N,), dtype=F32, device=x.device)
    check(_lib.load().clibd_l2norm_fwd(x.data_ptr(), N, D, y.data_ptr(), inv.data_ptr(), _stream()), "l2norm_fwd")
    return y, inv


def l2norm_bwd(dy: torch.Tensor, y: torch.Tensor, inv: torch.Tensor) -> torch.Tensor:
    _chk(dy, F32, "dy")
    _chk(y, F32, "y")
    _chk(inv, F32, "inv")
    N, D = y.shape
    dx = torch.empty_like(y)
    check(_lib.load().clibd_l2norm_bwd(dy.data_ptr(), y.data_ptr(), inv.data_ptr(), N, D, dx.data_ptr(), _stream()), "l2norm_bwd")
    return dx


def softce_workspace(Nx: int, N: int, D: int, device) -> torch.Tensor:
    nbytes = _lib.load().clibd_softce_workspace_bytes(Nx, N, D)
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def softce_rows_fwd(x, y, labels, row0: int, scale: torch.Tensor, loss_sum: torch.Tensor, ws: torch.Tensor) -> None:
    """`scale` is a 1-element fp32 DEVICE tensor (no host sync on the temperature)."""
    _chk(scale, F32, "scale")
    _chk(x, F32, "x")
    _chk(y, F32, "y")
    _chk(labels, I64, "labels")
    _chk(loss_sum, F32, "loss_sum")
    Nx, D = x.shape
    N = y.shape[0]
    if y.shape[1] != D or labels.numel() != N:
        raise ValueError("softce_rows_fwd: shapes")
    check(_lib.load().clibd_softce_rows_fwd(x.data_ptr(), y.data_ptr(), labels.data_ptr(), Nx, N, D, row0, scale.data_ptr(),
                                            loss_sum.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "softce_rows_fwd")


def softce_rows_bwd(labels, Nx, N, D, row0, scale, weight, dx, dy, dscale, ws, weight_scale=None) -> None:
    _chk(labels, I64, "labels")
    _chk(scale, F32, "scale")
    _chk(dx, F32, "dx")
    _chk(dy, F32, "dy")
    if tuple(dx.shape) != (Nx, D) or tuple(dy.shape) != (N, D):
        raise ValueError("softce_rows_bwd: shapes")
    if dscale is not None:
        _chk(dscale, F32, "dscale")
    check(_lib.load().clibd_softce_rows_bwd(labels.data_ptr(), Nx, N, D, row0, scale.data_ptr(), float(weight), _p(weight_scale), dx.data_ptr(), dy.data_ptr(),
                                            _p(dscale), ws.data_ptr(), ws.numel(), _stream()), "softce_rows_bwd")


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0) -> None:
    for nm, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, F32, nm)
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise ValueError("adamw_step: size mismatch")
    check(_lib.load().clibd_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, float(lr), float(beta1), float(beta2),
                                       float(eps), float(weight_decay), int(step), float(grad_scale), _stream()), "adamw_step")


def adam_l2_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0) -> None:
    """torch.optim.Adam(weight_decay=...) on a flat bucket: the decay is L2 added to the gradient (include/clibd_hip_simclr.h)."""
    for nm, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, F32, nm)
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise ValueError("adam_l2_step: size mismatch")
    check(_lib.load().clibd_adam_l2_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, float(lr), float(beta1), float(beta2),
                                         float(eps), float(weight_decay), int(step), float(grad_scale), _stream()), "adam_l2_step")


def grad_norm_workspace(n: int, device) -> torch.Tensor:
    nbytes = _lib.load().clibd_grad_norm_workspace_bytes(int(n))
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def grad_norm(g: torch.Tensor, record: torch.Tensor, ws: torch.Tensor, grad_scale: float = 1.0, max_norm: Optional[float] = None,
              skip_nonfinite: bool = False) -> None:
    """The L2 norm of the flat fp32 gradient `g` times `grad_scale`, in a fixed order (include/clibd_hip_optim.h).  `record` is a 16-byte
    device buffer the caller zeroed once, int32 [4]: [0] the norm and [1] the clip coefficient as fp32 bits (`record.view(torch.float32)`),
    [2] skip_now, [3] the running count of skips.  max_norm=None: no clipping (coefficient 1)."""
    _chk(g, F32, "g")
    _chk(record, torch.int32, "record")
    if g.dim() != 1 or record.numel() != 4:
        raise ValueError("grad_norm: g is flat, record is int32 [4]")
    check(_lib.load().clibd_grad_norm(g.data_ptr(), g.numel(), float(grad_scale), 0.0 if max_norm is None else float(max_norm),
                                      int(bool(skip_nonfinite)), record.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "grad_norm")


def grad_norm_div(g: torch.Tensor, record: torch.Tensor, ws: torch.Tensor, divisor: Optional[torch.Tensor], grad_scale: float = 1.0,
                  max_norm: Optional[float] = None, skip_nonfinite: bool = False) -> None:
    """`grad_norm` with a divisor on the device (include/clibd_hip_accum.h): `divisor` fp32 [1] or None; with d = max(divisor, 1) the record
    gets total_norm = grad_scale * sqrt(sum g^2) / d and coef = clip(total_norm) / d, so the grouped updates, which multiply the gradient
    by grad_scale * coef, apply the averaged and clipped gradient of an accumulation window.  None or 1: `grad_norm`'s record bit for bit.
    The workspace is `grad_norm_workspace`'s."""
    _chk(g, F32, "g")
    _chk(record, torch.int32, "record")
    if g.dim() != 1 or record.numel() != 4:
        raise ValueError("grad_norm_div: g is flat, record is int32 [4]")
    if divisor is not None:
        _chk(divisor, F32, "divisor")
        if divisor.numel() != 1:
            raise ValueError("grad_norm_div: divisor is fp32 [1]")
    check(_lib.load().clibd_grad_norm_div(g.data_ptr(), g.numel(), float(grad_scale), 0.0 if max_norm is None else float(max_norm),
                                          int(bool(skip_nonfinite)), _p(divisor), record.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "grad_norm_div")


def _step_groups(entry, what, p, g, m, v, groups, beta1, beta2, eps, step, grad_scale, record):
    import ctypes

    for nm, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, F32, nm)
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise ValueError(f"{what}: size mismatch")
    if record is not None:
        _chk(record, torch.int32, "record")
        if record.numel() != 4:
            raise ValueError(f"{what}: record is int32 [4]")
    groups = list(groups)
    table = (_lib.OptimGroup * max(len(groups), 1))(*[_lib.OptimGroup(int(f), float(lr), float(wd)) for f, lr, wd in groups])
    check(entry(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, ctypes.cast(table, ctypes.c_void_p), len(groups), float(beta1),
                float(beta2), float(eps), int(step), float(grad_scale), _p(record), _stream()), what)


def adamw_step_groups(p, g, m, v, groups, beta1, beta2, eps, step, grad_scale=1.0, record=None) -> None:
    """`adamw_step` with per-group hyperparameters and the clip / skip record of `grad_norm`: `groups` is a list of at most 8
    (first element, lr, weight_decay), first ascending from 0 in multiples of 64; the gradient is g * (grad_scale * coef); a set skip flag
    leaves p, m and v untouched.  record=None: no clipping, no skip.  The table travels in the kernel arguments: no copy to the device."""
    _step_groups(_lib.load().clibd_adamw_step_groups, "adamw_step_groups", p, g, m, v, groups, beta1, beta2, eps, step, grad_scale, record)


def adam_l2_step_groups(p, g, m, v, groups, beta1, beta2, eps, step, grad_scale=1.0, record=None) -> None:
    """`adam_l2_step` with per-group hyperparameters and the clip / skip record (see `adamw_step_groups`)."""
    _step_groups(_lib.load().clibd_adam_l2_step_groups, "adam_l2_step_groups", p, g, m, v, groups, beta1, beta2, eps, step, grad_scale, record)


def ntxent_workspace(N: int, D: int, device) -> torch.Tensor:
    nbytes = _lib.load().clibd_ntxent_workspace_bytes(N, D)
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def ntxent_fwd(f: torch.Tensor, inv_temperature: float, loss: torch.Tensor, ws: torch.Tensor, top1: Optional[torch.Tensor] = None) -> None:
    """NT-Xent over the [2b, D] raw features `f` (rows i and i + b are the two views of sample i): `loss` and `top1` are 1-element
    device tensors that are overwritten; `ws` (ntxent_workspace) carries the row statistics to ntxent_bwd."""
    _chk(f, F32, "f")
    _chk(loss, F32, "loss")
    if top1 is not None:
        _chk(top1, I32, "top1")
    if f.dim() != 2:
        raise ValueError("ntxent_fwd: expected [2b, D] features")
    N, D = f.shape
    check(_lib.load().clibd_ntxent_fwd(f.data_ptr(), N, D, float(inv_temperature), loss.data_ptr(), _p(top1), ws.data_ptr(), ws.numel(),
                                       _stream()), "ntxent_fwd")


def ntxent_bwd(f: torch.Tensor, inv_temperature: float, df: torch.Tensor, ws: torch.Tensor, dloss: Optional[torch.Tensor] = None) -> None:
    """d loss / d f into `df` (overwritten), times the device scalar `dloss` when given; must follow ntxent_fwd on the same `ws`."""
    _chk(f, F32, "f")
    _chk(df, F32, "df")
    if dloss is not None:
        _chk(dloss, F32, "dloss")
    if f.dim() != 2 or df.shape != f.shape:
        raise ValueError("ntxent_bwd: shapes")
    N, D = f.shape
    check(_lib.load().clibd_ntxent_bwd(f.data_ptr(), N, D, float(inv_temperature), _p(dloss), df.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream()), "ntxent_bwd")


def topk_ip(q: torch.Tensor, keys: torch.Tensor, k: int = 5):
    """Exact fp32 inner-product top-k (faiss.IndexFlatIP.search): returns (similarities fp32 [Q,k], indices int64 [Q,k]).
    Streaming: scores never leave the MFMA accumulators' running top-8 lists (no [Q,Nk] matrix)."""
    _chk(q, F32, "q")
    _chk(keys, F32, "keys")
    Q, D = q.shape
    Nk = keys.shape[0]
    if keys.shape[1] != D:
        raise ValueError("topk_ip: dimension mismatch")
    idx = torch.empty((Q, k), dtype=I64, device=q.device)
    sim = torch.empty((Q, k), dtype=F32, device=q.device)
    lib = _lib.load()
    ws = torch.empty((max(int(lib.clibd_topk_ip_workspace_bytes(Q, Nk)), 16),), dtype=torch.uint8, device=q.device)
    check(lib.clibd_topk_ip(q.data_ptr(), keys.data_ptr(), Q, Nk, D, k, idx.data_ptr(), sim.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "topk_ip")
    return sim, idx


class KeyBank:
    """A key bank prepared once for the pre-filtered search: the fp32 keys, their bf16 image and max ||key|| (clibd_topk_prepare_keys).
    The reference builds one faiss.IndexFlatIP per key set and searches it with every query batch (util/util.py:521-528)."""

    MAX_KEYS, MAX_D = 1 << 24, 2048   # the C entry points refuse beyond these too (topk.hip: TK_FAST_MAX_KEYS / TK_FAST_MAX_D)

    def __init__(self, keys: torch.Tensor):
        _chk(keys, F32, "keys")
        Nk, D = keys.shape
        if D % 64 != 0 or D > self.MAX_D or Nk >= self.MAX_KEYS:
            raise ValueError("KeyBank: the pre-filtered search needs D % 64 == 0, D <= 2048 and fewer than 2^24 keys (use topk_ip)")
        self.keys = keys
        self.keys_bf16 = torch.empty((Nk, D), dtype=BF16, device=keys.device)
        self.max_norm = torch.empty((1,), dtype=F32, device=keys.device)
        check(_lib.load().clibd_topk_prepare_keys(keys.data_ptr(), Nk, D, self.keys_bf16.data_ptr(), self.max_norm.data_ptr(), _stream()),
              "topk_prepare_keys")


def topk_ip_fast(q: torch.Tensor, bank: "KeyBank", k: int = 5):
    """clibd_topk_ip_fast: the top-k of `topk_ip` — same indices, same similarities, bit for bit — from bf16 approximate scores
    followed by an exact re-score of every key within the rigorous error band of the k-th best.  Returns (sim, idx, overflow):
    overflow int32 [Q] flags the queries whose candidate lists were full inside the band (their rows are unspecified; `topk_search`
    re-runs them through the exact kernel)."""
    _chk(q, F32, "q")
    Q, D = q.shape
    Nk = bank.keys.shape[0]
    if bank.keys.shape[1] != D:
        raise ValueError("topk_ip_fast: dimension mismatch")
    idx = torch.empty((Q, k), dtype=I64, device=q.device)
    sim = torch.empty((Q, k), dtype=F32, device=q.device)
    ovf = torch.empty((Q,), dtype=I32, device=q.device)
    lib = _lib.load()
    ws = torch.empty((int(lib.clibd_topk_ip_fast_workspace_bytes(Q, Nk, D)),), dtype=torch.uint8, device=q.device)
    check(lib.clibd_topk_ip_fast(q.data_ptr(), bank.keys.data_ptr(), bank.keys_bf16.data_ptr(), bank.max_norm.data_ptr(), Q, Nk, D, k, idx.data_ptr(),
                                 sim.data_ptr(), ovf.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "topk_ip_fast")
    return sim, idx, ovf


def kmer_tokenize(seq_u8: torch.Tensor, k: int = 5) -> torch.Tensor:
    """uint8 [B,L] ('N'-padded ASCII) -> int64 [B, 1 + L/k] token ids."""
    _chk(seq_u8, torch.uint8, "seq_u8")
    B, L = seq_u8.shape
    out = torch.empty((B, 1 + L // k), dtype=I64, device=seq_u8.device)
    check(_lib.load().clibd_kmer_tokenize(seq_u8.data_ptr(), B, L, k, out.data_ptr(), _stream()), "kmer_tokenize")
    return out


def image_transform(data: torch.Tensor, xforms: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed RGB HWC uint8 pixels `data` [N] + per-image records `xforms` int32 [B, 18] (struct clibd_image_xform; built by
    clibd_amd.augment) -> fp32 [B,3,224,224]: the dataset's Resize / crop / flip / rotation chain (clibd_image_transform_u8).
    The records are validated on the host when they are built; the kernel reads no byte outside `data` whatever they hold."""
    _chk(data, torch.uint8, "data")
    _chk(xforms, I32, "xforms")
    if data.dim() != 1 or data.numel() == 0:
        raise ValueError("image_transform: data must be a non-empty 1-D uint8 tensor")
    if xforms.dim() != 2 or xforms.shape[1] != 18 or xforms.shape[0] == 0 or xforms.device != data.device:
        raise ValueError("image_transform: xforms must be int32 [B, 18] on the data's device")
    B = xforms.shape[0]
    lib = _lib.load()
    need = int(lib.clibd_image_transform_workspace_bytes(B))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((need,), dtype=torch.uint8, device=data.device)
    out = torch.empty((B, 3, 224, 224), dtype=F32, device=data.device)
    check(lib.clibd_image_transform_u8(data.data_ptr(), data.numel(), xforms.data_ptr(), B, out.data_ptr(), workspace.data_ptr(),
                                       workspace.numel(), _stream()), "image_transform_u8")
    return out


def jpeg_decode(streams: torch.Tensor, plans: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor, total_blocks: int,
                status: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, phases: int = 3) -> torch.Tensor:
    """Baseline JPEG decode on the device (clibd_jpeg_decode_u8): `streams` uint8 [n] (the eligible streams, packed), `plans` uint8
    [B, 4096] (struct clibd_jpeg_record, built by clibd_amd.augment), `offsets` int64 [>= B] -> RGB HWC uint8 pixels of image i at
    out[offsets[i]:].  Returns the int32 [B] status (0: decoded; otherwise the slice is zero, or untouched for a record the plan left to
    the host).  phases: 1 entropy decode, 2 reconstruction, 3 both.  The kernels read and write nothing outside the buffers given here
    whatever the streams and records hold."""
    for t, dt, name in ((streams, torch.uint8, "streams"), (plans, torch.uint8, "plans"), (offsets, I64, "offsets"), (out, torch.uint8, "out")):
        _chk(t, dt, name)
        if t.device != out.device:
            raise ValueError("jpeg_decode: every tensor must be on one device")
    if plans.dim() != 2 or plans.shape[1] != 4096 or plans.shape[0] == 0 or offsets.numel() < plans.shape[0]:
        raise ValueError("jpeg_decode: plans must be uint8 [B, 4096] with one offset per image")
    B = plans.shape[0]
    lib = _lib.load()
    need = int(lib.clibd_jpeg_workspace_bytes(int(total_blocks)))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=out.device)
    if status is None:
        status = torch.empty((B,), dtype=I32, device=out.device)
    _chk(status, I32, "status")
    check(lib.clibd_jpeg_decode_u8(streams.data_ptr(), streams.numel(), plans.data_ptr(), B, out.data_ptr(), out.numel(), offsets.data_ptr(),
                                   status.data_ptr(), workspace.data_ptr(), workspace.numel(), int(total_blocks), int(phases), _stream()),
          "jpeg_decode_u8")
    return status


def simclr_views(data: torch.Tensor, xforms: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed RGB HWC uint8 pixels `data` [N] + one record per view `xforms` int32 [n, 16] (struct clibd_view_xform; built by
    clibd_amd.simclr_views) -> fp32 [n,3,224,224]: crop / flip / colour jitter / grayscale / blur of the SimCLR pipeline
    (clibd_simclr_views_u8).  The records are validated on the host when they are built; a bad one yields a zero image and the
    kernels read no byte outside `data` whatever the records hold.  workspace: a uint8 device buffer to reuse (grown when short)."""
    _chk(data, torch.uint8, "data")
    _chk(xforms, I32, "xforms")
    if data.dim() != 1 or data.numel() == 0:
        raise ValueError("simclr_views: data must be a non-empty 1-D uint8 tensor")
    if xforms.dim() != 2 or xforms.shape[1] != 16 or xforms.shape[0] == 0 or xforms.device != data.device:
        raise ValueError("simclr_views: xforms must be int32 [n, 16] on the data's device")
    n = xforms.shape[0]
    lib = _lib.load()
    need = int(lib.clibd_simclr_views_workspace_bytes(n))
    if workspace is None or workspace.numel() < need:
        workspace = _workspace("simclr_views", need, data.device)
    else:
        _chk(workspace, torch.uint8, "workspace")
    out = torch.empty((n, 3, 224, 224), dtype=F32, device=data.device)
    check(lib.clibd_simclr_views_u8(data.data_ptr(), data.numel(), xforms.data_ptr(), n, out.data_ptr(), workspace.data_ptr(),
                                    workspace.numel(), _stream()), "simclr_views_u8")
    return out


def topk_label_hits(idx: torch.Tensor, key_labels: torch.Tensor, query_labels: torch.Tensor, class_offset, k_list, segment: Optional[torch.Tensor] = None,
                    nseg: int = 1):
    """clibd_topk_label_hits: score a finished search against per-level class ids.  idx int64 [Q, kmax] (a search's output),
    key_labels int32 [Nk, L], query_labels int32 [Q, L], class_offset: L + 1 ints (host), k_list: strictly ascending ints <= kmax,
    segment: optional int32 [Q] in [0, nseg).  Returns (first_hit [Q, L], level_hits [nseg, n_k, L], class_hits [nseg, n_k, C],
    class_count [nseg, C]), int32 device tensors.  Reads one error word back (a host sync): an index outside [0, Nk), a query label
    outside its level's range or a segment outside [0, nseg) raises ValueError."""
    _chk(idx, I64, "idx")
    _chk(key_labels, I32, "key_labels")
    _chk(query_labels, I32, "query_labels")
    if idx.dim() != 2 or key_labels.dim() != 2 or query_labels.dim() != 2:
        raise ValueError("topk_label_hits: idx, key_labels and query_labels must be 2-D")
    Q, kmax = idx.shape
    Nk, L = key_labels.shape
    if tuple(query_labels.shape) != (Q, L):
        raise ValueError(f"topk_label_hits: query_labels must be [{Q}, {L}], got {list(query_labels.shape)}")
    off = (C.c_int32 * (L + 1))(*[int(v) for v in class_offset]) if len(class_offset) == L + 1 else None
    if off is None:
        raise ValueError(f"topk_label_hits: class_offset needs L + 1 = {L + 1} entries")
    ks = (C.c_int32 * len(k_list))(*[int(k) for k in k_list])
    if segment is not None:
        _chk(segment, I32, "segment")
        if tuple(segment.shape) != (Q,):
            raise ValueError("topk_label_hits: segment must be [Q]")
    n_k, Ccls = len(k_list), int(class_offset[-1])
    dev = idx.device
    first_hit = torch.empty((Q, L), dtype=I32, device=dev)
    level_hits = torch.empty((nseg, n_k, L), dtype=I32, device=dev)
    class_hits = torch.empty((nseg, n_k, max(Ccls, 1)), dtype=I32, device=dev)
    class_count = torch.empty((nseg, max(Ccls, 1)), dtype=I32, device=dev)
    err = torch.empty((1,), dtype=I32, device=dev)
    lib = _lib.load()
    check(lib.clibd_topk_label_hits(idx.data_ptr(), Q, kmax, key_labels.data_ptr(), Nk, query_labels.data_ptr(), L, off, ks, n_k, _p(segment), nseg,
                                    first_hit.data_ptr(), level_hits.data_ptr(), class_hits.data_ptr(), class_count.data_ptr(), err.data_ptr(),
                                    _stream()), "topk_label_hits")
    e = int(err.item())
    if e:
        what = [m for b, m in ((1, "a key index outside [0, Nk)"), (2, "a query label outside its level's class range"), (4, "a segment outside [0, nseg)"))
                if e & b]
        raise ValueError(f"topk_label_hits: {', '.join(what)}")
    return first_hit, level_hits, class_hits, class_count


def eval_pair_features(img: torch.Tensor, dna: torch.Tensor):
    """clibd_eval_pair_features: (averaged fp32 [N, D], concatenated fp32 [N, 2D]) of two embeddings, as the reference's
    get_features_and_label builds them (np.mean([img, dna], 0) rounded to fp32, np.concatenate((img, dna), 1)); unnormalised."""
    _chk(img, F32, "img")
    _chk(dna, F32, "dna")
    if img.dim() != 2 or img.shape != dna.shape:
        raise ValueError("eval_pair_features: img and dna must be 2-D of one shape")
    N, D = img.shape
    avg = torch.empty((N, D), dtype=F32, device=img.device)
    cat = torch.empty((N, 2 * D), dtype=F32, device=img.device)
    check(_lib.load().clibd_eval_pair_features(img.data_ptr(), dna.data_ptr(), N, D, avg.data_ptr(), cat.data_ptr(), _stream()), "eval_pair_features")
    return avg, cat


def threshold_sweep_hits(conf: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, key_labels_a: torch.Tensor, key_labels_b: torch.Tensor,
                         query_labels: torch.Tensor, thresholds: torch.Tensor, k_list, segment: Optional[torch.Tensor] = None, nseg: int = 1):
    """clibd_threshold_sweep_hits: top-k label hits of the merged prediction (A's key where (double)conf > t, else B's) at EVERY threshold.
    conf fp32 [Q, m], idx_a / idx_b int64 [Q, m], key_labels_a int32 [Nka, L], key_labels_b int32 [Nkb, L], query_labels int32 [Q, L],
    thresholds fp64 [T] (device), k_list: strictly ascending ints <= m, segment: optional int32 [Q] in [0, nseg).  Returns level_hits
    int32 [T, nseg, n_k, L] (device).  Reads one error word back (a host sync): an index outside its key table, a negative query label
    or a segment outside [0, nseg) raises ValueError."""
    _chk(conf, F32, "conf")
    _chk(idx_a, I64, "idx_a")
    _chk(idx_b, I64, "idx_b")
    _chk(key_labels_a, I32, "key_labels_a")
    _chk(key_labels_b, I32, "key_labels_b")
    _chk(query_labels, I32, "query_labels")
    _chk(thresholds, torch.float64, "thresholds")
    if conf.dim() != 2 or idx_a.shape != conf.shape or idx_b.shape != conf.shape:
        raise ValueError("threshold_sweep_hits: conf, idx_a and idx_b must be 2-D of one shape")
    if key_labels_a.dim() != 2 or key_labels_b.dim() != 2 or query_labels.dim() != 2 or thresholds.dim() != 1:
        raise ValueError("threshold_sweep_hits: label tables must be 2-D and thresholds 1-D")
    Q, m = conf.shape
    Nka, L = key_labels_a.shape
    Nkb = key_labels_b.shape[0]
    if key_labels_b.shape[1] != L or tuple(query_labels.shape) != (Q, L):
        raise ValueError(f"threshold_sweep_hits: key_labels_b must be [Nkb, {L}] and query_labels [{Q}, {L}]")
    if segment is not None:
        _chk(segment, I32, "segment")
        if tuple(segment.shape) != (Q,):
            raise ValueError("threshold_sweep_hits: segment must be [Q]")
    T, n_k = thresholds.numel(), len(k_list)
    ks = (C.c_int32 * n_k)(*[int(k) for k in k_list])
    dev = conf.device
    level_hits = torch.empty((T, nseg, n_k, L), dtype=I32, device=dev)
    err = torch.empty((1,), dtype=I32, device=dev)
    lib = _lib.load()
    ws = torch.empty((max(int(lib.clibd_threshold_sweep_workspace_bytes(Q, L)), 16),), dtype=torch.uint8, device=dev)
    check(lib.clibd_threshold_sweep_hits(conf.data_ptr(), idx_a.data_ptr(), idx_b.data_ptr(), Q, m, key_labels_a.data_ptr(), Nka, key_labels_b.data_ptr(),
                                         Nkb, query_labels.data_ptr(), L, _p(segment), nseg, thresholds.data_ptr(), T, ks, n_k, level_hits.data_ptr(),
                                         err.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "threshold_sweep_hits")
    e = int(err.item())
    if e:
        what = [msg for b, msg in ((1, "a key index outside its key table"), (2, "a negative query label"), (4, "a segment outside [0, nseg)")) if e & b]
        raise ValueError(f"threshold_sweep_hits: {', '.join(what)}")
    return level_hits


def threshold_merge(conf: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, Nka: int, Nkb: int, threshold: float):
    """clibd_threshold_merge: (merged_idx int64 [Q, m], from_a int32 [Q]) at one threshold: idx_a[q, j] where (double)conf[q, j] > threshold,
    Nka + idx_b[q, j] otherwise (indices into the concatenated label table); bit j of from_a set when rank j came from A.  Reads one
    error word back (a host sync): an index outside its key table raises ValueError."""
    _chk(conf, F32, "conf")
    _chk(idx_a, I64, "idx_a")
    _chk(idx_b, I64, "idx_b")
    if conf.dim() != 2 or idx_a.shape != conf.shape or idx_b.shape != conf.shape:
        raise ValueError("threshold_merge: conf, idx_a and idx_b must be 2-D of one shape")
    Q, m = conf.shape
    dev = conf.device
    merged = torch.empty((Q, m), dtype=I64, device=dev)
    from_a = torch.empty((Q,), dtype=I32, device=dev)
    err = torch.empty((1,), dtype=I32, device=dev)
    check(_lib.load().clibd_threshold_merge(conf.data_ptr(), idx_a.data_ptr(), idx_b.data_ptr(), Q, m, int(Nka), int(Nkb), float(threshold),
                                            merged.data_ptr(), from_a.data_ptr(), err.data_ptr(), _stream()), "threshold_merge")
    if int(err.item()):
        raise ValueError("threshold_merge: a key index outside its key table")
    return merged, from_a


# ------------------------------------------------------------------------------------------------ full fine-tune mode (f4)
def layernorm_param_grads(dy: torch.Tensor, x: torch.Tensor, stats: torch.Tensor, dgamma: torch.Tensor, dbeta: torch.Tensor,
                          drop: Optional[Drop] = None, ordered: bool = False) -> None:
    """dgamma += sum_m dy*xhat, dbeta += sum_m dy  (dy [M,H] bf16 or fp32; x fp32 [M,H]; stats fp32 [M,2])."""
    if dy.dtype not in (BF16, F32):
        raise TypeError("dy: expected bf16 or fp32")
    _chk(dy, dy.dtype, "dy", contiguous=False)
    _chk(x, F32, "x"); _chk(stats, F32, "stats"); _chk(dgamma, F32, "dgamma"); _chk(dbeta, F32, "dbeta")
    M, H = x.shape
    if tuple(dy.shape) != (M, H) or stats.numel() != 2 * M or dgamma.numel() != H or dbeta.numel() != H:
        raise ValueError("layernorm_param_grads: shape mismatch")
    lib = _lib.load()
    ws = _workspace("ln_param", int(lib.clibd_layernorm_param_grads_workspace_bytes(M, H)), x.device) if ordered else None
    check(lib.clibd_layernorm_param_grads(dy.data_ptr(), int(dy.dtype == F32), _rowmajor(dy, "dy"), x.data_ptr(), stats.data_ptr(), M, H,
                                          dgamma.data_ptr(), dbeta.data_ptr(), *_drop_args(drop), *_ws_args(ws), _stream()), "layernorm_param_grads")


def batch_sum(x: torch.Tensor, out: torch.Tensor, ordered: bool = False) -> None:
    """out[...] += x.sum(0)   (x fp32 [B, ...], out fp32 with x.shape[1:] elements).  ordered: per-chunk partials, summed in chunk order."""
    _chk(x, F32, "x"); _chk(out, F32, "out")
    B = x.shape[0]
    R = x.numel() // B
    if out.numel() != R:
        raise ValueError("batch_sum: out must have x.numel() / B elements")
    lib = _lib.load()
    ws = _workspace("batch_sum", int(lib.clibd_batch_sum_workspace_bytes(B, R)), x.device) if ordered else None
    check(lib.clibd_batch_sum_f32(x.data_ptr(), B, R, out.data_ptr(), *_ws_args(ws), _stream()), "batch_sum")


def bert_embed_bwd(ids: torch.Tensor, token_type: Optional[torch.Tensor], de: torch.Tensor, dword: Optional[torch.Tensor],
                   dtype_table: Optional[torch.Tensor], ordered: bool = False) -> None:
    """Scatter the embedding gradient de [M,H] into the word table (by ids) and the token-type table (accumulating).
    ordered: the word table through a stable sort of (id, row) and per-id sums in row order, the token-type table (at most two types)
    through per-block partials."""
    _chk(ids, torch.int64, "ids"); _chk(de, F32, "de")
    M, H = de.shape
    if ids.numel() != M:
        raise ValueError("bert_embed_bwd: ids / de mismatch")
    if token_type is not None:
        _chk(token_type, torch.int64, "token_type")
    vocab = dword.shape[0] if dword is not None else 1
    tv = dtype_table.shape[0] if dtype_table is not None else 1
    for t, n in ((dword, "dword"), (dtype_table, "dtype")):
        if t is not None:
            _chk(t, F32, n)
    if ordered and tv > 2:
        raise _not_ordered(f"bert_embed_bwd with {tv} token types")
    lib = _lib.load()
    ws = _workspace("embed", int(lib.clibd_bert_embed_bwd_workspace_bytes(M, H, vocab, tv)), de.device) if ordered else None
    check(lib.clibd_bert_embed_bwd(ids.data_ptr(), _p(token_type), de.data_ptr(), M, H, vocab, tv, _p(dword), _p(dtype_table), *_ws_args(ws),
                                   _stream()), "bert_embed_bwd")


def slice_rows_cast_bf16(x: torch.Tensor, s0: int, s1: int) -> torch.Tensor:
    """x fp32 [B,S,H] -> bf16 [B*(s1-s0), H]: rows s0..s1-1 of every sequence."""
    _chk(x, F32, "x")
    B, S, H = x.shape
    out = torch.empty((B * (s1 - s0), H), dtype=BF16, device=x.device)
    check(_lib.load().clibd_slice_rows_cast_bf16(x.data_ptr(), B, S, H, s0, s1, out.data_ptr(), _stream()), "slice_rows_cast_bf16")
    return out


def dropout_apply(x: torch.Tensor, drop: Drop) -> torch.Tensor:
    """x * dropout_factor(seed, flat element index)  (fp32): the gradient through y = dropout(.)."""
    _chk(x, F32, "x")
    y = torch.empty_like(x)
    check(_lib.load().clibd_dropout_apply_f32(x.data_ptr(), x.numel(), y.data_ptr(), drop.seed, drop.thr16, drop.scale, _stream()), "dropout_apply")
    return y


def gemm_tn_splitk(a: torch.Tensor, b: torch.Tensor, out_f32: torch.Tensor, accumulate: bool = True, colsum: Optional[torch.Tensor] = None,
                   ordered: bool = False, b_scale: Optional[float] = None) -> bool:
    """out[Na,Nb] (+)= a[M,Na]^T @ b[M,Nb], both operands read in place (clibd_gemm_bf16_tn_splitk): the weight gradient
    dW = dy^T x without transposes; colsum (fp32 [Na]) += column sums of a in the same pass (the bias gradient).
    Returns False (nothing launched) when the shape is outside the kernel's.  ordered: the column sums per M-slice, summed in slice order.
    b as float8_e4m3fn with b_scale (> 0; required): out (+)= a^T @ (b * b_scale) (clibd_gemm_fp8b_tn_splitk) — the weight gradient of a
    GEMM whose forward consumed x as e4m3(x * sa), with b_scale = 1 / sa."""
    b8 = b.dtype == FP8
    if b8:
        if b_scale is None or not (float(b_scale) > 0.0) or not math.isfinite(float(b_scale)):
            raise ValueError("gemm_tn_splitk: an e4m3 b needs b_scale > 0 (finite)")
        _chk(b, FP8, "b", contiguous=False)
    elif b_scale is not None:
        raise ValueError("gemm_tn_splitk: b_scale goes with an e4m3 b only")
    else:
        _chk(b, BF16, "b", contiguous=False)
    _chk(a, BF16, "a", contiguous=False); _chk(out_f32, F32, "out_f32")
    M, Na = a.shape
    Nb = b.shape[1]
    if b.shape[0] != M or tuple(out_f32.shape) != (Na, Nb):
        raise ValueError("gemm_tn_splitk: shape mismatch")
    if M % 128 or M < 256 or Na % 256 or Nb % 256:
        return False
    if colsum is not None:
        _chk(colsum, F32, "colsum")
        if colsum.numel() != Na:
            raise ValueError("gemm_tn_splitk: colsum must have Na elements")
    lib = _lib.load()
    ws = _workspace("splitk", int(lib.clibd_gemm_splitk_workspace_bytes(Na, Nb)), a.device)   # shared with the NT mode
    cws = _workspace("tn_colsum", int(lib.clibd_gemm_tn_colsum_workspace_bytes(M, Na)), a.device) if ordered and colsum is not None else None
    fn, scale = (lib.clibd_gemm_fp8b_tn_splitk, (float(b_scale),)) if b8 else (lib.clibd_gemm_bf16_tn_splitk, ())
    rc = fn(a.data_ptr(), _rowmajor(a, "a"), b.data_ptr(), _rowmajor(b, "b"), *scale, M, Na, Nb, out_f32.data_ptr(), Nb, int(accumulate), _p(colsum),
            *_ws_args(ws), *_ws_args(cws), _stream())
    if rc != 0 and b"shape not supported" in (lib.clibd_last_error() or b""):
        return False    # declined before anything was enqueued: the caller takes the transpose + NT path
    check(rc, "gemm_fp8b_tn_splitk" if b8 else "gemm_bf16_tn_splitk")
    return True


def gemm_nt_splitk(a: torch.Tensor, w: torch.Tensor, out_f32: torch.Tensor, accumulate: bool = True) -> bool:
    """out (+)= a @ w.T for a long contraction and few output tiles (weight gradients), through the split-K workspace path
    of the 256x256 kernel.  Returns False (nothing launched) when the shape is outside that path — use gemm_nt(split_k=)."""
    _chk(a, BF16, "a", contiguous=False); _chk(w, BF16, "w", contiguous=False); _chk(out_f32, F32, "out_f32")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(out_f32.shape) != (M, N):
        raise ValueError("gemm_nt_splitk: shape mismatch")
    if N % 256 or K % 128 or K < 512:
        return False
    lib = _lib.load()
    ws = _workspace("splitk", int(lib.clibd_gemm_splitk_workspace_bytes(M, N)), a.device)   # shared with the TN mode
    rc = lib.clibd_gemm_bf16_nt_splitk(a.data_ptr(), _rowmajor(a, "a"), w.data_ptr(), _rowmajor(w, "w"), M, N, K, out_f32.data_ptr(), N,
                                       int(accumulate), *_ws_args(ws), _stream())
    if rc != 0 and b"shape not supported" in (lib.clibd_last_error() or b""):
        return False    # declined before anything was enqueued: the caller uses gemm_nt(split_k=)
    check(rc, "gemm_bf16_nt_splitk")
    return True


# ------------------------------------------------------------------------------------------------ linear-probe classifier (include/clibd_hip_classifier.h)
def _linear_f32_ws(B: int, Ccls: int, D: int, device) -> torch.Tensor:
    return _workspace("linear_f32", int(_lib.load().clibd_linear_f32_workspace_bytes(B, Ccls, D)), device)


def linear_f32_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x w^T + bias at split-bf16 accuracy (clibd_linear_f32_fwd): x fp32 [B, D], w fp32 [C, D], bias fp32 [C] or None -> fp32 [B, C]
    (`out`: a 2-D fp32 tensor with unit inner stride to write into)."""
    _chk(x, F32, "x"); _chk(w, F32, "w")
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise ValueError("linear_f32_fwd: expected x [B, D] and w [C, D]")
    B, D = x.shape
    Ccls = w.shape[0]
    if bias is not None:
        _chk(bias, F32, "bias")
        if bias.numel() != Ccls:
            raise ValueError("linear_f32_fwd: bias must have C elements")
    if out is None:
        out = torch.empty((B, Ccls), dtype=F32, device=x.device)
    else:
        _chk(out, F32, "out", contiguous=False)
        if tuple(out.shape) != (B, Ccls):
            raise ValueError(f"linear_f32_fwd: out must be [{B}, {Ccls}]")
    ws = _linear_f32_ws(B, Ccls, D, x.device)
    check(_lib.load().clibd_linear_f32_fwd(x.data_ptr(), w.data_ptr(), _p(bias), B, Ccls, D, out.data_ptr(), _rowmajor(out, "out"), ws.data_ptr(),
                                           ws.numel(), _stream()), "linear_f32_fwd")
    return out


def linear_f32_bwd(dout: torch.Tensor, x: torch.Tensor, w: torch.Tensor, need_dx: bool = True, need_dw: bool = True, need_db: bool = True):
    """(dx [B, D] = dout w, dw [C, D] = dout^T x, db [C] = dout.sum(0)) through the split images (clibd_linear_f32_bwd); an output that is
    not needed is None.  Fixed summation orders: two calls give the same bits."""
    _chk(dout, F32, "dout"); _chk(x, F32, "x"); _chk(w, F32, "w")
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1] or tuple(dout.shape) != (x.shape[0], w.shape[0]):
        raise ValueError("linear_f32_bwd: expected dout [B, C], x [B, D] and w [C, D]")
    B, D = x.shape
    Ccls = w.shape[0]
    dev = x.device
    dx = torch.empty((B, D), dtype=F32, device=dev) if need_dx else None
    dw = torch.empty((Ccls, D), dtype=F32, device=dev) if need_dw else None
    db = torch.empty((Ccls,), dtype=F32, device=dev) if need_db else None
    ws = _linear_f32_ws(B, Ccls, D, dev)
    check(_lib.load().clibd_linear_f32_bwd(dout.data_ptr(), x.data_ptr(), w.data_ptr(), B, Ccls, D, _p(dx), _p(dw), _p(db), ws.data_ptr(), ws.numel(),
                                           _stream()), "linear_f32_bwd")
    return dx, dw, db


# ------------------------------------------------------------------------------------------------ feature-tower linear layers (include/clibd_hip_mlp.h)
def mlp_linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x w^T + bias) at split-bf16 accuracy in one launch (clibd_mlp_linear_fwd): x fp32 [B, K], w fp32 [N, K], bias fp32 [N] or
    None -> fp32 [B, N]; act = ReLU when `relu`.  K % 4 == 0, N % 16 == 0, both <= 4096."""
    _chk(x, F32, "x"); _chk(w, F32, "w")
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise ValueError("mlp_linear_fwd: expected x [B, K] and w [N, K]")
    B, K = x.shape
    N = w.shape[0]
    if bias is not None:
        _chk(bias, F32, "bias")
        if bias.numel() != N:
            raise ValueError("mlp_linear_fwd: bias must have N elements")
    if out is None:
        out = torch.empty((B, N), dtype=F32, device=x.device)
    else:
        _chk(out, F32, "out")
        if tuple(out.shape) != (B, N):
            raise ValueError(f"mlp_linear_fwd: out must be [{B}, {N}]")
    check(_lib.load().clibd_mlp_linear_fwd(x.data_ptr(), w.data_ptr(), _p(bias), B, N, K, int(bool(relu)), out.data_ptr(), _stream()), "mlp_linear_fwd")
    return out


def mlp_linear_dgrad(dy: torch.Tensor, w: torch.Tensor, h: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(dy w) * [h > 0] in one launch (clibd_mlp_linear_dgrad): dy fp32 [B, N], w fp32 [N, K], h fp32 [B, K] = the post-ReLU activation
    that fed this layer (None: no mask) -> dx fp32 [B, K]."""
    _chk(dy, F32, "dy"); _chk(w, F32, "w")
    if dy.dim() != 2 or w.dim() != 2 or w.shape[0] != dy.shape[1]:
        raise ValueError("mlp_linear_dgrad: expected dy [B, N] and w [N, K]")
    B, N = dy.shape
    K = w.shape[1]
    if h is not None:
        _chk(h, F32, "h")
        if tuple(h.shape) != (B, K):
            raise ValueError(f"mlp_linear_dgrad: h must be [{B}, {K}]")
    if out is None:
        out = torch.empty((B, K), dtype=F32, device=dy.device)
    else:
        _chk(out, F32, "out")
        if tuple(out.shape) != (B, K):
            raise ValueError(f"mlp_linear_dgrad: out must be [{B}, {K}]")
    check(_lib.load().clibd_mlp_linear_dgrad(dy.data_ptr(), w.data_ptr(), _p(h), B, N, K, out.data_ptr(), _stream()), "mlp_linear_dgrad")
    return out


def mlp_linear_wgrad(dy: torch.Tensor, x: torch.Tensor, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None,
                     accumulate: bool = False, need_db: bool = True):
    """dw [N, K] (+)= dy^T x and db [N] (+)= dy.sum(0) in one launch (clibd_mlp_linear_wgrad): dy fp32 [B, N], x fp32 [B, K].
    dw / db: fp32 tensors to write (accumulate=True: to add to, e.g. views of the trainer's flat gradient bucket); None allocates
    (db only when need_db).  One summation order: two calls give the same bits.  Returns (dw, db)."""
    _chk(dy, F32, "dy"); _chk(x, F32, "x")
    if dy.dim() != 2 or x.dim() != 2 or x.shape[0] != dy.shape[0]:
        raise ValueError("mlp_linear_wgrad: expected dy [B, N] and x [B, K]")
    B, N = dy.shape
    K = x.shape[1]
    if accumulate and (dw is None or (need_db and db is None)):
        raise ValueError("mlp_linear_wgrad: accumulate needs the tensors to add to")
    if dw is None:
        dw = torch.empty((N, K), dtype=F32, device=dy.device)
    if db is None and need_db:
        db = torch.empty((N,), dtype=F32, device=dy.device)
    _chk(dw, F32, "dw")
    if tuple(dw.shape) != (N, K):
        raise ValueError(f"mlp_linear_wgrad: dw must be [{N}, {K}]")
    if db is not None:
        _chk(db, F32, "db")
        if db.numel() != N:
            raise ValueError("mlp_linear_wgrad: db must have N elements")
    check(_lib.load().clibd_mlp_linear_wgrad(dy.data_ptr(), x.data_ptr(), B, N, K, dw.data_ptr(), _p(db), int(bool(accumulate)), _stream()),
          "mlp_linear_wgrad")
    return dw, db


_ce_err: dict = {}   # device -> the int32 error word of ce_rows_fwd (sticky: bit 0 = a target outside [0, C))


def ce_error_word(device) -> torch.Tensor:
    """The device word that ce_rows_fwd ORs its target-range flag into.  Reading it is a host synchronisation, so nothing on the
    training path does; `ce_rows_fwd(check=True)` and a caller at an epoch's end may."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    e = _ce_err.get(dev)
    if e is None:
        e = _ce_err[dev] = torch.zeros((1,), dtype=I32, device=dev)
    return e


def ce_rows_fwd(logits: torch.Tensor, target: torch.Tensor, check: bool = False):   # `check` shadows _lib.check here: the calls below name the module
    """nn.CrossEntropyLoss() forward (mean over rows, integer targets; clibd_ce_rows_fwd): logits fp32 [B, C] with unit inner stride,
    target int64 [B] -> (loss fp32 [1], lse fp32 [B]) on the device.  A target outside [0, C) contributes nothing and sets bit 0 of
    `ce_error_word`; with check=True the word is read back (a host sync), cleared, and such a target raises ValueError."""
    _chk(logits, F32, "logits", contiguous=False); _chk(target, I64, "target")
    ld = _rowmajor(logits, "logits")
    B, Ccls = logits.shape
    if tuple(target.shape) != (B,):
        raise ValueError(f"ce_rows_fwd: target must be [{B}]")
    dev = logits.device
    loss = torch.empty((1,), dtype=F32, device=dev)
    lse = torch.empty((B,), dtype=F32, device=dev)
    err = ce_error_word(dev)
    lib = _lib.load()
    ws = _workspace("ce_rows", int(lib.clibd_ce_rows_workspace_bytes(B)), dev)
    _lib.check(lib.clibd_ce_rows_fwd(logits.data_ptr(), ld, target.data_ptr(), B, Ccls, lse.data_ptr(), loss.data_ptr(), err.data_ptr(), ws.data_ptr(),
                                     ws.numel(), _stream()), "ce_rows_fwd")
    if check:
        e = int(err.item())
        err.zero_()
        if e & 1:
            raise ValueError(f"ce_rows_fwd: a target outside [0, {Ccls})")
    return loss, lse


def ce_rows_bwd(logits: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, dloss: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d loss / d logits [B, C] = dloss / B * (softmax - onehot) (clibd_ce_rows_bwd); dloss: a 1-element fp32 device tensor or None (1).
    Rows whose target lies outside [0, C) are zero."""
    _chk(logits, F32, "logits", contiguous=False); _chk(target, I64, "target"); _chk(lse, F32, "lse")
    ld = _rowmajor(logits, "logits")
    B, Ccls = logits.shape
    if tuple(target.shape) != (B,) or lse.numel() != B:
        raise ValueError(f"ce_rows_bwd: target and lse must be [{B}]")
    if dloss is not None:
        _chk(dloss, F32, "dloss")
        if dloss.numel() != 1:
            raise ValueError("ce_rows_bwd: dloss must have one element")
    d = torch.empty((B, Ccls), dtype=F32, device=logits.device)
    _lib.check(_lib.load().clibd_ce_rows_bwd(logits.data_ptr(), ld, target.data_ptr(), lse.data_ptr(), B, Ccls, _p(dloss), d.data_ptr(), Ccls, _stream()),
               "ce_rows_bwd")
    return d


def softmax_topk(logits: torch.Tensor, k: int = 5):
    """torch.topk(F.softmax(logits, -1), k, sorted=True) (clibd_softmax_topk): (conf fp32 [B, k], idx int64 [B, k]); equal values resolve
    to the lower index.  1 <= k <= 8, and k > C raises as in torch."""
    _chk(logits, F32, "logits", contiguous=False)
    ld = _rowmajor(logits, "logits")
    B, Ccls = logits.shape
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError("softmax_topk: k must be in 1..8")
    if k > Ccls:
        raise RuntimeError("softmax_topk: selected index k out of range")
    conf = torch.empty((B, k), dtype=F32, device=logits.device)
    idx = torch.empty((B, k), dtype=I64, device=logits.device)
    _lib.check(_lib.load().clibd_softmax_topk(logits.data_ptr(), ld, B, Ccls, k, conf.data_ptr(), idx.data_ptr(), _stream()), "softmax_topk")
    return conf, idx


# ---- the embedding analysis (include/clibd_hip_analysis.h) ----------------------------------------------------------------------------
def _host_seg(seg, name: str):
    """run offsets as (host int32 array, C): the C entries validate the host copy before they launch; the caller uploads the device copy"""
    import numpy as np

    host = np.ascontiguousarray(seg.detach().cpu().numpy() if torch.is_tensor(seg) else np.asarray(seg), dtype=np.int32)
    if host.ndim != 1 or host.size < 2:
        raise ValueError(f"{name}: seg must be a 1-D array of C + 1 run offsets")
    return host, host.size - 1


def silhouette_workspace_bytes(N: int, col_chunk: int = 0) -> int:
    return int(_lib.load().clibd_silhouette_workspace_bytes(int(N), int(col_chunk)))


def silhouette_samples(x: torch.Tensor, seg, col_chunk: int = 0) -> torch.Tensor:
    """sklearn's silhouette_samples(x, labels) for rows already ordered by cluster (clibd_silhouette_samples): x fp32 [N, D], D a multiple
    of 32; seg [C + 1] the run offsets (host array or tensor); returns s fp32 [N] in the order of x's rows.  Fewer than 2 or more than
    N - 1 clusters raises ValueError with sklearn's condition."""
    _chk(x, F32, "x")
    if x.dim() != 2:
        raise ValueError("silhouette_samples: x must be [N, D]")
    N, D = x.shape
    host, Ccl = _host_seg(seg, "silhouette_samples")
    if not 2 <= Ccl <= N - 1:
        raise ValueError(f"Number of labels is {Ccl}. Valid values are 2 to n_samples - 1 (inclusive)")
    if D % 32 != 0:
        raise ValueError("silhouette_samples: D must be a multiple of 32 (zero pad the columns)")
    seg_d = torch.from_numpy(host).to(x.device)
    need = silhouette_workspace_bytes(N, col_chunk)
    if need == 0:
        raise ValueError("silhouette_samples: col_chunk must be 0 or a positive multiple of 64 and N at most 2^24")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    out = torch.empty(N, dtype=F32, device=x.device)
    check(_lib.load().clibd_silhouette_samples(x.data_ptr(), N, D, seg_d.data_ptr(), host.ctypes.data, Ccl, int(col_chunk), out.data_ptr(),
                                               ws.data_ptr(), need, _stream()), "silhouette_samples")
    return out


def same_label_nearest(q: torch.Tensor, k: torch.Tensor, seg, qclass: torch.Tensor):
    """The distance from each query to the nearest key of its own class (clibd_same_label_nearest): q fp32 [Nq, D], k fp32 [Nk, D] grouped by
    class with run offsets seg [C + 1], qclass int32 [Nq] in [0, C) or -1.  Returns (dist fp32 [Nq], arg int32 [Nq]); the lowest key row
    wins a tie; an empty class or -1 gives (+inf, -1)."""
    _chk(q, F32, "q", contiguous=False)
    _chk(k, F32, "k", contiguous=False)
    _chk(qclass, I32, "qclass")
    ldq, ldk = _rowmajor(q, "q"), _rowmajor(k, "k")
    if q.shape[1] != k.shape[1]:
        raise ValueError("same_label_nearest: q and k differ in width")
    Nq, D = q.shape
    Nk = k.shape[0]
    if qclass.shape != (Nq,):
        raise ValueError("same_label_nearest: qclass must be [Nq]")
    host, Ccl = _host_seg(seg, "same_label_nearest")
    seg_d = torch.from_numpy(host).to(q.device)
    dist = torch.empty(Nq, dtype=F32, device=q.device)
    arg = torch.empty(Nq, dtype=I32, device=q.device)
    check(_lib.load().clibd_same_label_nearest(q.data_ptr(), ldq, k.data_ptr(), ldk, Nq, Nk, D, seg_d.data_ptr(), host.ctypes.data, Ccl,
                                               qclass.data_ptr(), dist.data_ptr(), arg.data_ptr(), _stream()), "same_label_nearest")
    return dist, arg


def confusion_counts(true_code: torch.Tensor, pred_code: torch.Tensor, num_classes: int) -> torch.Tensor:
    """int32 [C, C] counts, rows = true (clibd_confusion_counts); a sample whose true or predicted code is -1 is skipped."""
    _chk(true_code, I32, "true_code")
    _chk(pred_code, I32, "pred_code")
    if true_code.dim() != 1 or true_code.shape != pred_code.shape:
        raise ValueError("confusion_counts: true_code and pred_code must be 1-D and of equal length")
    Ccl = int(num_classes)
    out = torch.empty((Ccl, Ccl), dtype=I32, device=true_code.device)
    check(_lib.load().clibd_confusion_counts(true_code.data_ptr(), pred_code.data_ptr(), true_code.numel(), Ccl, out.data_ptr(), _stream()),
          "confusion_counts")
    return out


# ---- the attention rollout (include/clibd_hip_rollout.h) --------------------------------------------------------------------------------
FUSE_MEAN, FUSE_MAX, FUSE_MIN = 0, 1, 2


def rollout_ld(S: int) -> int:
    """the row stride of a fused map: S rounded up to 4, so that a row takes 16-byte stores"""
    return (int(S) + 3) // 4 * 4


def attn_fused_maps(qkv: torch.Tensor, B: int, S: int, heads: int, fusion: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fuse_h softmax(q_h k_h^T / 8) of one layer (clibd_attn_fused_maps): qkv bf16 [B * S, 3 * 64 * heads] as clibd_attention_fwd reads it;
    returns (or fills) fp32 [B, S, rollout_ld(S)], whose columns >= S are padding."""
    _chk(qkv, BF16, "qkv")
    B, S, heads = int(B), int(S), int(heads)
    if qkv.dim() != 2 or tuple(qkv.shape) != (B * S, 3 * 64 * heads):
        raise ValueError(f"attn_fused_maps: qkv must be [{B * S}, {3 * 64 * heads}] (head dim 64)")
    if fusion not in (FUSE_MEAN, FUSE_MAX, FUSE_MIN):
        raise ValueError("attn_fused_maps: fusion must be FUSE_MEAN, FUSE_MAX or FUSE_MIN")
    ld = rollout_ld(S)
    if out is None:
        out = torch.empty((B, S, ld), dtype=F32, device=qkv.device)
    _chk(out, F32, "out")
    if tuple(out.shape) != (B, S, ld):
        raise ValueError(f"attn_fused_maps: out must be [{B}, {S}, {ld}]")
    check(_lib.load().clibd_attn_fused_maps(qkv.data_ptr(), B, S, heads, int(fusion), out.data_ptr(), ld, _stream()), "attn_fused_maps")
    return out


def rollout_discard_(maps: torch.Tensor, S: int, k: int) -> torch.Tensor:
    """In place on maps fp32 [..., S, ld] (clibd_rollout_discard): per map the k smallest of its S * S entries become 0, except entry [0, 0],
    which still counts among the k; ties at the k-th value go in ascending flat index.  Returns the selection record, int64 [n, 4]: the bits of
    the k-th smallest value, the entries below it, the entries equal to it that were taken, k."""
    _chk(maps, F32, "maps")
    S, k = int(S), int(k)
    if maps.dim() < 2 or maps.shape[-2] != S or maps.shape[-1] < S:
        raise ValueError("rollout_discard_: maps must be [..., S, ld] with ld >= S")
    if not 0 <= k <= S * S:
        raise ValueError("rollout_discard_: k must be in 0..S*S")
    ld = maps.shape[-1]
    n = maps.numel() // (S * ld)
    need = int(_lib.load().clibd_rollout_discard_workspace_bytes(n))
    ws = torch.empty(need // 4, dtype=I32, device=maps.device)
    check(_lib.load().clibd_rollout_discard(maps.data_ptr(), n, S, ld, k, ws.data_ptr(), need, _stream()), "rollout_discard")
    return ws.view(n, 4).to(I64) & 0xFFFFFFFF


def rollout_chain(maps: torch.Tensor, S: int) -> torch.Tensor:
    """The chain of the discarded maps (clibd_rollout_chain): maps fp32 [L, B, S, ld] in the order of application; returns fp32 [B, S - 1],
    row 0 of the product of the column-normalised (F + I) / 2 without its first entry, divided by its maximum."""
    _chk(maps, F32, "maps")
    S = int(S)
    if maps.dim() != 4 or maps.shape[2] != S or maps.shape[3] < S:
        raise ValueError("rollout_chain: maps must be [L, B, S, ld] with ld >= S")
    if S < 2:
        raise ValueError("rollout_chain: S must be at least 2")
    L, B, _, ld = maps.shape
    out = torch.empty((B, S - 1), dtype=F32, device=maps.device)
    check(_lib.load().clibd_rollout_chain(maps.data_ptr(), L, B, S, ld, out.data_ptr(), _stream()), "rollout_chain")
    return out


# ---- the INSECT / BZSL workflow (include/clibd_hip_insect.h) ---------------------------------------------------------------------------
def class_mean(x: torch.Tensor, labels: torch.Tensor, num_classes: int, transposed: bool = False, out: Optional[torch.Tensor] = None,
               error: Optional[torch.Tensor] = None):
    """The class means in numpy's order (clibd_class_mean_f32): x fp32 [N, D] with unit inner stride (a row stride above D is taken as it
    is), labels int32 [N].  Returns (mean, count int32 [C], error int32 [1]): mean fp32 [C, D], or [D, C] with transposed=True (`out`: a
    2-D fp32 tensor of that shape with unit inner stride to write into).  mean[c] = ((x[i1] + x[i2]) + ...) / n over the rows of class c
    in ascending order, bit for bit np.sum(rows, axis=0) / len(rows); an empty class is a zero row.  A label outside [0, C) is skipped
    and sets bit 0 of `error` (a fresh zero word unless one is passed); nothing is read back here."""
    _chk(x, F32, "x", contiguous=False)
    _chk(labels, I32, "labels")
    ld_x = _rowmajor(x, "x")
    N, D = x.shape
    Ccls = int(num_classes)
    if tuple(labels.shape) != (N,):
        raise ValueError(f"class_mean: labels must be [{N}]")
    if N < 1 or D < 1 or not 1 <= Ccls <= 65536 or N * D >= 2 ** 31:
        raise ValueError("class_mean: need N >= 1, D >= 1, 1 <= C <= 65536 and N * D < 2^31")
    if N > 1 and ld_x < D:
        raise ValueError("class_mean: the rows of x overlap")
    dev = x.device
    shape = (D, Ccls) if transposed else (Ccls, D)
    if out is None:
        out = torch.empty(shape, dtype=F32, device=dev)
    else:
        _chk(out, F32, "out", contiguous=False)
        if tuple(out.shape) != shape:
            raise ValueError(f"class_mean: out must be {list(shape)}")
    ld_mean = _rowmajor(out, "out")
    count = torch.empty((Ccls,), dtype=I32, device=dev)
    if error is None:
        error = torch.zeros((1,), dtype=I32, device=dev)
    else:
        _chk(error, I32, "error")
    lib = _lib.load()
    ws = _workspace("class_mean", int(lib.clibd_class_mean_workspace_bytes(N, Ccls)), dev)
    check(lib.clibd_class_mean_f32(x.data_ptr(), max(ld_x, D), labels.data_ptr(), N, Ccls, D, out.data_ptr(), max(ld_mean, shape[1]), int(bool(transposed)),
                                   count.data_ptr(), error.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "class_mean_f32")
    return out, count, error


def logits_topk(logits: torch.Tensor, k: int = 5):
    """torch.sort(logits, dim=1, descending=True, stable=True) cut to k columns (clibd_logits_topk): (val fp32 [B, k] — the logits
    themselves —, idx int64 [B, k]); equal values resolve to the lower index, -inf is a value like any other, NaN is not supported.
    1 <= k <= 8, and k > C raises as in softmax_topk."""
    _chk(logits, F32, "logits", contiguous=False)
    ld = _rowmajor(logits, "logits")
    B, Ccls = logits.shape
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError("logits_topk: k must be in 1..8")
    if k > Ccls:
        raise RuntimeError("logits_topk: selected index k out of range")
    val = torch.empty((B, k), dtype=F32, device=logits.device)
    idx = torch.empty((B, k), dtype=I64, device=logits.device)
    check(_lib.load().clibd_logits_topk(logits.data_ptr(), max(ld, Ccls), B, Ccls, k, val.data_ptr(), idx.data_ptr(), _stream()), "logits_topk")
    return val, idx


# ---- masked-k-mer pre-training (include/clibd_hip_mlm.h) ---------------------------------------------------------------------------------
MLM_IGNORE = -100   # CLIBD_MLM_IGNORE: torch's ignore_index


def mlm_mask(ids: torch.Tensor, seed: int, n_mask: int, mask_id: int = 0, unk_id: int = 2):
    """The position sampler (clibd_mlm_mask): ids int64 [B, S] -> (masked int64 [B, S], rows int32 [B * n_mask], targets int64 [B * n_mask],
    n_valid int32 [1]).  n_mask positions per sequence, never position 0, padding k-mers (unk_id) last; rows = b * S + s ascending;
    a target is the original id, or MLM_IGNORE where that was unk_id.  Nothing is read back."""
    _chk(ids, I64, "ids")
    if ids.dim() != 2:
        raise ValueError("mlm_mask: ids must be [B, S]")
    B, S = ids.shape
    n_mask = int(n_mask)
    if B < 1 or not 2 <= S <= 256 or not 1 <= n_mask <= S - 1:
        raise ValueError("mlm_mask: need B >= 1, 2 <= S <= 256 and 1 <= n_mask <= S - 1")
    dev = ids.device
    masked = torch.empty_like(ids)
    rows = torch.empty((B * n_mask,), dtype=I32, device=dev)
    targets = torch.empty((B * n_mask,), dtype=I64, device=dev)
    n_valid = torch.empty((1,), dtype=I32, device=dev)
    check(_lib.load().clibd_mlm_mask(ids.data_ptr(), B, S, int(seed) & 0xFFFFFFFF, n_mask, int(mask_id), int(unk_id), masked.data_ptr(), rows.data_ptr(),
                                     targets.data_ptr(), n_valid.data_ptr(), _stream()), "mlm_mask")
    return masked, rows, targets, n_valid


def rows_gather(x: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """x bf16 [M, H] (H % 8 == 0), rows int32 [R] -> x[rows] bf16 [R, H] (clibd_rows_gather_bf16)."""
    _chk(x, BF16, "x"); _chk(rows, I32, "rows")
    if x.dim() != 2 or rows.dim() != 1 or rows.numel() < 1 or x.shape[1] % 8:
        raise ValueError("rows_gather: x must be [M, H] with H % 8 == 0 and rows a non-empty vector")
    M, H = x.shape
    out = torch.empty((rows.numel(), H), dtype=BF16, device=x.device)
    check(_lib.load().clibd_rows_gather_bf16(x.data_ptr(), M, H, rows.data_ptr(), rows.numel(), out.data_ptr(), _stream()), "rows_gather_bf16")
    return out


def rows_scatter(src: torch.Tensor, rows: torch.Tensor, M: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The transpose of rows_gather (clibd_rows_scatter_bf16): bf16 [M, H] with out[rows[i]] = src[i] and zeros in every other row; the
    call writes all of `out` (a fresh tensor unless one is passed).  The rows must be distinct: a repeated index is not detected."""
    _chk(src, BF16, "src"); _chk(rows, I32, "rows")
    if src.dim() != 2 or tuple(rows.shape) != (src.shape[0],) or src.shape[0] < 1 or src.shape[1] % 8:
        raise ValueError("rows_scatter: src must be [R, H] with H % 8 == 0 and rows [R]")
    R, H = src.shape
    if out is None:
        out = torch.empty((int(M), H), dtype=BF16, device=src.device)
    else:
        _chk(out, BF16, "out")
        if tuple(out.shape) != (int(M), H):
            raise ValueError(f"rows_scatter: out must be [{int(M)}, {H}]")
    check(_lib.load().clibd_rows_scatter_bf16(src.data_ptr(), rows.data_ptr(), R, int(M), H, out.data_ptr(), _stream()), "rows_scatter_bf16")
    return out


def mlm_ce_(logits: torch.Tensor, V: int, targets: torch.Tensor, n_valid: torch.Tensor):
    """Cross-entropy over the first V columns of bf16 logits [R, ld] (unit inner stride, ld % 8 == 0), IN PLACE (clibd_mlm_ce_bf16): returns
    (loss fp32 [1], correct int32 [1], row_loss fp32 [R]) and leaves d loss / d logits in `logits` — (softmax - onehot) / max(n_valid, 1),
    exactly 0 in rows whose target is MLM_IGNORE and in the columns from V on.  A target outside {MLM_IGNORE} U [0, V) sets bit 0 of
    `ce_error_word` and counts as ignored."""
    _chk(logits, BF16, "logits", contiguous=False); _chk(targets, I64, "targets"); _chk(n_valid, I32, "n_valid")
    ld = _rowmajor(logits, "logits")
    R = logits.shape[0]
    V = int(V)
    if R < 1 or not 1 <= V <= min(8192, logits.shape[1]) or tuple(targets.shape) != (R,) or n_valid.numel() != 1:
        raise ValueError("mlm_ce_: need R >= 1, 1 <= V <= min(8192, columns), targets [R] and a one-element n_valid")
    dev = logits.device
    row_loss = torch.empty((R,), dtype=F32, device=dev)
    loss = torch.empty((1,), dtype=F32, device=dev)
    correct = torch.empty((1,), dtype=I32, device=dev)
    check(_lib.load().clibd_mlm_ce_bf16(logits.data_ptr(), ld, targets.data_ptr(), R, V, n_valid.data_ptr(), row_loss.data_ptr(), loss.data_ptr(),
                                        correct.data_ptr(), ce_error_word(dev).data_ptr(), _stream()), "mlm_ce_bf16")
    return loss, correct, row_loss


# ---- masked-LM labels: compaction and BERT's sampler (include/clibd_hip_mlm_labels.h) ---------------------------------------------------------
MLM_PAD_ROW = -1   # CLIBD_MLM_PAD_ROW: rows_gather reads a zero row for it, rows_scatter writes nothing
_mlm_overflow = {}


def mlm_overflow_word(device) -> torch.Tensor:
    """The device word mlm_compact_labels ORs its overflow bit into unless the caller passes its own.  Sticky; reading it is a host
    synchronisation, so nothing on the training path does."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    w = _mlm_overflow.get(dev)
    if w is None:
        w = _mlm_overflow[dev] = torch.zeros((1,), dtype=I32, device=dev)
    return w


def mlm_label_capacity(M: int, p: Optional[float] = None) -> int:
    """The row capacity of the vocabulary head for M = B * S positions, a multiple of 64.  p=None: M rounded up (always enough).  A
    probability p: M * min(1, p + 6 sqrt(p (1 - p) / M)) rounded up — six binomial standard deviations over the mean number of chosen
    positions when every one of the M is eligible."""
    M = int(M)
    if M < 1:
        raise ValueError("mlm_label_capacity: M must be positive")
    full = (M + 63) // 64 * 64
    if p is None:
        return full
    if not 0.0 <= p <= 1.0:
        raise ValueError("mlm_label_capacity: p must be in [0, 1]")
    n = math.ceil(M * min(1.0, p + 6.0 * math.sqrt(p * (1.0 - p) / M)))
    return min(full, max(64, (n + 63) // 64 * 64))


def mlm_compact_labels(labels: torch.Tensor, V: int, r_cap: Optional[int] = None, overflow: Optional[torch.Tensor] = None):
    """HF-style labels int64 [...] (MLM_IGNORE = not labelled) -> (rows int32 [r_cap], targets int64 [r_cap], n_labelled int32 [1])
    (clibd_mlm_compact_labels): the labelled flat positions ascending, then padding (MLM_PAD_ROW / MLM_IGNORE).  r_cap: a multiple of 64
    in 64 .. M rounded up; None = M rounded up.  More labelled positions than r_cap set bit 0 of `overflow` (int32 [1], sticky; default
    mlm_overflow_word) and leave the correct prefix; a label outside [0, V) sets bit 0 of ce_error_word.  Nothing is read back."""
    _chk(labels, I64, "labels")
    M = labels.numel()
    r_cap = mlm_label_capacity(M) if r_cap is None else int(r_cap)
    if M < 1 or M > 1 << 24 or r_cap < 64 or r_cap % 64 or r_cap > (M + 63) // 64 * 64 or int(V) < 1:
        raise ValueError("mlm_compact_labels: need 1 <= M <= 2^24, V >= 1 and r_cap a multiple of 64 in 64 .. M rounded up to 64")
    dev = labels.device
    if overflow is None:
        overflow = mlm_overflow_word(dev)
    else:
        _chk(overflow, I32, "overflow")
    L = _lib.load()
    rows = torch.empty((r_cap,), dtype=I32, device=dev)
    targets = torch.empty((r_cap,), dtype=I64, device=dev)
    n = torch.empty((1,), dtype=I32, device=dev)
    ws = torch.empty((L.clibd_mlm_compact_workspace_bytes(M),), dtype=torch.uint8, device=dev)
    check(L.clibd_mlm_compact_labels(labels.data_ptr(), M, int(V), r_cap, rows.data_ptr(), targets.data_ptr(), n.data_ptr(), overflow.data_ptr(),
                                     ce_error_word(dev).data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "mlm_compact_labels")
    return rows, targets, n


def mlm_mask_bert(ids: torch.Tensor, attention_mask: Optional[torch.Tensor], V: int, seed: int, mlm_probability: float = 0.15, mask_id: int = 0,
                  special_ids=(0, 1, 2), replace=(0.8, 0.1, 0.1)):
    """BERT's Bernoulli sampler (clibd_mlm_mask_bert; the header has the rule): ids int64 [B, S], attention_mask [B, S] or None ->
    (masked int64 [B, S], labels int64 [B, S]).  `replace` = (P mask_id, P random non-special id, P unchanged), summing to 1."""
    _chk(ids, I64, "ids")
    if ids.dim() != 2:
        raise ValueError("mlm_mask_bert: ids must be [B, S]")
    B, S = ids.shape
    special = [int(s) for s in special_ids]
    if len(replace) != 3 or abs(sum(replace) - 1.0) > 1e-6 or min(replace) < 0:
        raise ValueError("mlm_mask_bert: replace = (mask, random, unchanged), non-negative, summing to 1")
    if B < 1 or S < 1 or len(special) > 8 or int(V) <= len(special) or not 0.0 <= mlm_probability <= 1.0:
        raise ValueError("mlm_mask_bert: need B, S >= 1, at most 8 special ids, V > their number and a probability in [0, 1]")
    am = None
    if attention_mask is not None:
        if tuple(attention_mask.shape) != (B, S) or not attention_mask.is_cuda:
            raise ValueError("mlm_mask_bert: attention_mask must be a device tensor [B, S]")
        am = attention_mask.to(I32).contiguous()
    masked, labels = torch.empty_like(ids), torch.empty_like(ids)
    sp = (C.c_int64 * max(len(special), 1))(*special)
    check(_lib.load().clibd_mlm_mask_bert(ids.data_ptr(), _p(am), B, S, int(V), int(seed) & 0xFFFFFFFF, float(mlm_probability), float(replace[0]),
                                          float(replace[1]), int(mask_id), C.cast(sp, C.c_void_p), len(special), masked.data_ptr(), labels.data_ptr(),
                                          _stream()), "mlm_mask_bert")
    return masked, labels
