"""Tower engines: forward + hand-derived backward of the three CLIBD encoders on the HIP kernels.

Each tower is ONE torch.autograd.Function (inputs = the trainable parameters, output = the tower's [B, D]
embedding): the forward enqueues the fused kernels layer by layer and keeps exactly the activations the
LoRA backward needs; the backward walks the layers in reverse (dgrad only for the frozen base weights,
rank-4 adapter gradients, head weight gradients).  Numerics follow torch.autocast(bf16) in the reference
(epoch/train_epoch.py:42-46): bf16 GEMM/attention operands with fp32 accumulation, fp32 residual stream,
fp32 LayerNorm / softmax statistics.

Reference arithmetic being replaced (all third-party model code the reference delegates to):
  ViT block        timm vision_transformer.Block       via model/image_encoder.py:106-107
  BERT layer       HF BertLayer (post-LN)              via model/dna_encoder.py:137, language_encoder.py:89
  LoRA             model/image_encoder.py:40-46, model/dna_encoder.py:75-77
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import List, Optional, Sequence

import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32


class NotSupportedYet(NotImplementedError):
    pass


# ---- numerics switches of the backward --------------------------------------------------------------------------------------------
# Explicit per-stack settings (`TransformerStack.numerics`, set through `SimpleCLIP.set_numerics(...)` / `Trainer(numerics=...)`);
# the environment variables only give the DEFAULT a stack is constructed with, so two trainers in one process can differ and a
# bench line / training state records which arithmetic produced it (`bench.py` config.numerics, `checkpoint.save_training_state`).
#
# residual_grad ("bf16" default | "fp32"; env CLIBD_RESIDUAL_GRAD).  Frozen-base (LoRA) backward: the gradient of the residual stream
#   travels between blocks as bf16 instead of fp32 — the LayerNorm backward then moves 10 instead of 16 bytes per element and the
#   BERT dgrad GEMMs join the stream with a bf16 add (CLIBD_ACT_ADD_AUX) instead of an fp32 read + write.  The reference's autograd
#   keeps this stream in fp32 (also under autocast); the extra rounding (one bf16 rounding per block-half: ~0.1 % rms each,
#   independent) is budgeted in DESIGN.md §4.  Full fine-tune mode (disable_lora) follows the same switch since round 4 — its bottom
#   layer still hands an fp32 gradient to the embedding backward; tests/test_model_gpu.py::test_full_finetune_residual_grad_streams_agree
#   gates the bf16 stream against the fp32 one on the same model.
# gelu_grad ("bf16" default | "u8" | "e4m7"; env CLIBD_GELU_GRAD).  gelu'(fc1 out) is all the MLP's backward needs (frozen fc1 / fc2 carry no
#   weight gradient that would want the activation), and it lies in [-0.129, 1.129].  "u8" keeps it as ONE BYTE per element
#   (CLIBD_ACT_GELU_SAVE_GRAD_U8, |error| <= 2.5e-3 everywhere; bf16's half-spacing is 2.0e-3 in [0.5, 1), 3.9e-3 in [1, 2), finer
#   below 0.5) and the fc2 dgrad multiplies by the decoded byte (CLIBD_ACT_MUL_AUX_U8): 50 GB less per step at b=2048, 285.1 -> 282.5
#   ms.  Gradient effect at full size: 5e-4 (ViT) / 4e-5 (BERT) relative, invisible against the oracle; on the tiny
#   fixtures the WORST per-tensor error moves by +-10 % (medians unchanged), which the tightest gate (x1.6 of the reference's own
#   autocast error) does not always absorb — so the default stays the bf16 form.  The fp8-forward mode always uses bf16.
#   Round 6: "e4m7" keeps the bf16 value of gelu' in TWELVE bits — sign, 4-bit exponent, bf16's 7 mantissa bits; gelu' lies in [-0.129, 1.129],
#   sixteen binades [2^-14, 2) cover it — so every bf16 gelu' of magnitude >= 2^-14 = 6.1e-5 is reproduced BIT FOR BIT and smaller ones
#   (pre-activations below about -4.55) become zero: the fc2 dgrad multiplies by the same operand as the bf16 form, at 1.5 instead of 2 bytes per
#   element on the fc1 forward's write and the fc2 dgrad's read (CLIBD_ACT_GELU_SAVE_GRAD_E12 / CLIBD_ACT_MUL_AUX_E12; tests/test_ops_gpu.py::
#   test_gelu_grad_e4m7_is_the_bf16_value, tests/test_model_gpu.py::test_gelu_grad_e4m7_towers_equal_the_bf16_form).  Numerically free — and a measured
#   NO-GO as the default: the step is 3.0 % SLOWER with it (294.9 against 286.3 ms, three interleaved pairs on one box, profiles/r06_exp_gelu_grad_e4m7.log).
#   The twelve-bit pack / unpack has no conversion instruction behind it (~100 VALU operations per row of eight columns where the bf16 form takes
#   four v_cvt_pk and the one-byte form eight v_cvt_pk_u8), and the GEMM's epilogue is exposed time: it roughly doubles the VALU work of the fc1
#   epilogue, which the 12.5 % fewer output bytes do not buy back; a hand-packed encode (v_pk_sub_u16 clamp on the bf16 pairs, ~32 operations per
#   row) would still cost more cycles than the bytes save.  Opt-in, for completeness of the byte ladder 2 / 1.5 / 1.
# attn_bwd ("2phase" default | "sp"; env CLIBD_ATTN_BWD).  "2phase" = the kernel that derives the softmax statistics itself and
#   evaluates every score twice; "sp" = single pass (ops.attention_bwd_sp; the training forward then also saves its per-layer output,
#   the rounding residual of that output and the log-sum-exp: 4 more bytes per element of activation memory per layer).  The
#   single-pass form needs full sequences without a key mask, S <= 224 and the bf16 forward; everything else (text tower, the
#   class-row-only last ViT block, fp8-forward mode) keeps the two-phase kernel.  Round 3 measurement: parity-green,
#   1.7 x fewer MFMAs and half the exponentials per head, but as built 1.17 - 1.24 x SLOWER — it stays opt-in.
# ln_fold ("off" default | "on"; env CLIBD_LN_FOLD; pre-LN stacks = the ViT, frozen base, bf16 forward).  A FORWARD switch: norm2 -> mlp.fc1 of a
#   block runs as the algebraic fold  fc1(LN(x)) = rstd (x . (gamma o W)^T - mean s) + b'  — the projection's epilogue also writes a bf16 copy
#   of the residual stream and per-slice row sums, a 5-us kernel turns those into (mean, rstd), and fc1 takes the copy and the gamma-scaled
#   weight image and applies the row terms in its epilogue: the LayerNorm's own HBM pass (6 bytes per element) disappears.  The bf16 rounding
#   moves from LN(x) to x; measured error of the fc1 pre-activation against fp64: the same (tools/ln_fold_study.py: ratio 1.00 at random
#   init, 1.2 with 100-sigma outlier channels).  The backward is the unchanged LayerNorm backward (same statistics).  DESIGN.md §3.1c.
# * dgrad (round 5, BASELINE.json configs[4]): "bf16" — the activation-gradient GEMMs on bf16 operands; "fp8" — the MLP pair and the attention
#   projection of every layer take their gradient operand as e4m3 with ONE power-of-two scale per token row (written by the LayerNorm backward
#   that produces it, from the row maximum it already holds; d(fc1 out) inherits the row scale times a per-layer constant derived from an l1 bound
#   on the fc2 weight, so nothing saturates and no history of maxima is kept) against the transposed frozen weight as e4m3 with one scale per
#   input channel, on v_mfma_f32_16x16x128_f8f6f4.  The QKV dgrad (its operand feeds the adapters' bf16 weight gradients), attention and every
#   weight gradient stay bf16.  Oracle study (full-size towers, tools/fp8_policy_study.py, profiles/r05_exp_fp8_dgrad_study.log): gradient cosine
#   against the bf16 dgrad 0.9998 on the training batch / 0.9875 on a fresh one with BOTH towers on it (MI355X, trained weights: 0.9998-1.0000 on
#   the mean-pooled towers, 0.987-0.9998 with the ViT's too; SimpleCLIP.enable_fp8_dgrad selects towers).  The bf16 residual-gradient stream only
#   (gelu' as bf16 or as its one-byte code); a call whose token count is not a multiple of 4 takes the bf16 GEMMs.  Round 6: also with TRAINABLE base
#   weights (disable_lora, the reference's final recipe) — the e4m3 weight images are re-made every step, the LayerNorm backward writes the e4m3 rows
#   AND the bf16 copy the weight gradient contracts (clibd_layernorm_bwd with dx_fp8 and dgamma / dbeta), the fc2 dgrad writes d(fc1 out) as e4m3 AND as bf16; every weight /
#   bias / LayerNorm gradient is the bf16 path's arithmetic on those copies.  DESIGN.md §3.1d.
NUMERICS_CHOICES = dict(residual_grad=("bf16", "fp32"), gelu_grad=("bf16", "u8", "e4m7"), attn_bwd=("2phase", "sp"), ln_fold=("off", "on"),
                        dgrad=("bf16", "fp8"))
_NUMERICS_ENV = dict(residual_grad="CLIBD_RESIDUAL_GRAD", gelu_grad="CLIBD_GELU_GRAD", attn_bwd="CLIBD_ATTN_BWD", ln_fold="CLIBD_LN_FOLD",
                     dgrad="CLIBD_DGRAD")


def default_deterministic() -> bool:
    """Deterministic training mode (opt-in; env CLIBD_DETERMINISTIC=1 gives a new stack / tower the default "on").  Not a numerics switch:
    it changes no arithmetic, only the order of the reductions that would otherwise end in float atomics (LayerNorm / bias / embedding
    parameter gradients, the adapters' gradients at token counts that are not whole 32-row slabs, split-K weight gradients): each takes a
    partials workspace and a fixed-order second kernel (ops.*(ordered=True)), so a training step repeats bit for bit on one GPU.  Kept out
    of NUMERICS_CHOICES (bench lines record those)."""
    return os.environ.get("CLIBD_DETERMINISTIC", "0") == "1"


def _ordered(on: bool) -> dict:
    """keyword arguments selecting the fixed-order form of an ops reduction: none at all when the mode is off (calls stay as they were)"""
    return {"ordered": True} if on else {}


def ln_param_grads(grads: dict, w, b, ordered: bool) -> dict:
    """keyword arguments of ops.layernorm_bwd that accumulate d(gamma), d(beta) of the LayerNorm (w, b) in the same pass: none when
    `grads` holds no bucket for them"""
    return dict(dgamma=grads[id(w)].view(-1), dbeta=grads[id(b)].view(-1), **_ordered(ordered)) if id(w) in grads else {}


def default_numerics() -> dict:
    """The settings a new stack starts with: the first choice of each switch unless its environment variable names another."""
    out = {}
    for k, choices in NUMERICS_CHOICES.items():
        v = os.environ.get(_NUMERICS_ENV[k], choices[0]).lower()
        out[k] = v if v in choices else choices[0]
    return out


def check_numerics(settings: dict) -> dict:
    for k, v in settings.items():
        if k not in NUMERICS_CHOICES:
            raise ValueError(f"unknown numerics switch {k!r} (known: {sorted(NUMERICS_CHOICES)})")
        if v not in NUMERICS_CHOICES[k]:
            raise ValueError(f"numerics switch {k}: {v!r} is not one of {NUMERICS_CHOICES[k]}")
    return settings


def _mul_aux_act(h, FF: int) -> int:
    """the fc2 dgrad's epilogue for the way gelu' was saved: bf16 [M,FF], one byte per element (uint8 [M,FF]) or the 12-bit e4m7 form (uint8 [M,3FF/2])"""
    if h.dtype == torch.uint8:
        return ops.ACT_MUL_AUX_E12 if h.shape[1] == 3 * FF // 2 else ops.ACT_MUL_AUX_U8
    return ops.ACT_MUL_AUX


@dataclass
class LoraParams:
    """The four adapter matrices of one layer (nn.Parameters, fp32): a_* [4,H], b_* [H,4]."""
    a_q: torch.nn.Parameter
    b_q: torch.nn.Parameter
    a_v: torch.nn.Parameter
    b_v: torch.nn.Parameter

    def tensors(self):
        return [self.a_q, self.b_q, self.a_v, self.b_v]


@dataclass
class LayerSpec:
    """Parameter handles of one transformer layer (fp32 masters living in the nn.Module tree)."""
    qkv_w: Sequence[torch.Tensor]   # one fused [3H,H] tensor or (q,k,v) [H,H] each
    qkv_b: Sequence[torch.Tensor]
    proj_w: torch.Tensor
    proj_b: torch.Tensor
    fc1_w: torch.Tensor
    fc1_b: torch.Tensor
    fc2_w: torch.Tensor
    fc2_b: torch.Tensor
    ln1_w: torch.Tensor             # ViT: norm1 (before attention).  BERT: attention.output.LayerNorm
    ln1_b: torch.Tensor
    ln2_w: torch.Tensor             # ViT: norm2 (before MLP).        BERT: output.LayerNorm
    ln2_b: torch.Tensor
    lora: Optional[LoraParams] = None

    def frozen(self):
        return [*self.qkv_w, *self.qkv_b, self.proj_w, self.proj_b, self.fc1_w, self.fc1_b, self.fc2_w, self.fc2_b, self.ln1_w,
                self.ln1_b, self.ln2_w, self.ln2_b]


class _LayerCache:
    """bf16 device images of one layer's frozen weights: W [N,K] for forward, W^T [K,N] for dgrad.
    fp8-forward mode adds the e4m3 forward images and their per-channel dequantisation factors (w*8, cs_*)."""
    __slots__ = ("wqkv", "wqkv_t", "bqkv", "wo", "wo_t", "bo", "w1", "w1_t", "b1", "w2", "w2_t", "b2", "g1", "be1", "g2", "be2",
                 "v_fwd", "v_bwd", "a_cat", "w_dt", "slot2", "wqkv8", "cs_qkv", "wo8", "cs_o", "w18", "cs_1", "w28", "cs_2",
                 "w1g", "s1", "b1f",   # ln_fold: bf16(gamma2 o W1), its row sums, b1 + W1 beta2
                 "wo_t8", "cs_ot", "w1_t8", "cs_1t", "w2_t8", "cs_2t", "c2")   # dgrad = fp8: e4m3 images of the transposed weights, c2 = d(fc1 out)'s fixed scale


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    return t if (t.dtype == F32 and t.is_contiguous()) else t.to(F32).contiguous()


def _rank_slots(lp: "LoraParams"):
    """The kernels carry the adapters as rank 4 + 4 (q and v in one MFMA k-slot of 8).  The reference accepts any r > 0
    (image_encoder.py:53; every shipped config uses 4): ranks 1-3 run zero-padded — A gets zero rows, B zero columns, the same
    product — and ranks above 4 as ceil(r / 4) such slots, rows / columns 4j .. 4j+3 of every adapter matrix
    (B A x = sum_j B_j A_j x): every slot after the first takes a pass of its own for its down-projection, rank update and gradients
    (TransformerStack._slot2_*; round 4: any r > 0, as the reference accepts — round 3 stopped at two slots, r <= 8).
    Returns [(a_q, a_v, b_q, b_v)] per slot, each [4,H] / [H,4] fp32."""
    a_q, a_v, b_q, b_v = _f32c(lp.a_q), _f32c(lp.a_v), _f32c(lp.b_q), _f32c(lp.b_v)
    r, H = a_q.shape

    def slot(lo):
        hi = min(lo + 4, r)
        k = hi - lo
        pa = lambda a: a[lo:hi].contiguous() if k == 4 else torch.cat([a[lo:hi], a.new_zeros((4 - k, H))], dim=0)
        pb = lambda b: (b[:, lo:hi] if k == 4 else torch.cat([b[:, lo:hi], b.new_zeros((H, 4 - k))], dim=1)).contiguous()
        return pa(a_q), pa(a_v), pb(b_q), pb(b_v)

    return [slot(lo) for lo in range(0, r, 4)]


class TransformerStack:
    """Shared machinery of the ViT (pre-LN) and BERT (post-LN) encoder stacks."""

    def __init__(self, layers: List[LayerSpec], hidden: int, heads: int, pre_ln: bool, eps: float):
        if heads < 1 or hidden % heads or hidden // heads not in self.HEAD_DIMS:
            raise NotSupportedYet(f"attention kernels are built for head_dim 64, 128 and 192 (hidden={hidden}, heads={heads})")
        if hidden % 64 or hidden > 1024:
            raise NotSupportedYet("hidden size must be a multiple of 64 and <= 1024")
        self.layers, self.H, self.heads, self.pre_ln, self.eps = layers, hidden, heads, pre_ln, eps
        self.dh = hidden // heads   # 64: attention.hip, every form.  128 / 192: attention_wide.hip (no key mask, no class-row-only form, no e4m3 output)
        self.FF = layers[0].fc1_w.shape[0]
        self._cache: List[_LayerCache] = []
        self._cache_key = None
        self.fp8 = None  # fp8-forward mode: [{site: activation scale}] per layer; see enable_fp8
        self._calib = None
        self.numerics = default_numerics()   # backward arithmetic switches (see NUMERICS_CHOICES above); set_numerics() changes them
        self.deterministic = default_deterministic()   # fixed-order reductions in the backward (see default_deterministic)
        self._c2, self._c2_age = None, 0   # dgrad = "fp8" under full fine-tune: the per-layer d(fc1 out) scales and how many refreshes old they are
        self.dgrad8_sites = ("mlp", "proj")   # dgrad = "fp8": which of the covered GEMMs take it ("mlp" = the fc2 -> fc1 pair, "proj"); tools/dgrad8_sites_study.py
        # True: a forward that saves nothing still runs the TRAINING forward's arithmetic — fc1 applies GELU to the bf16-rounded pre-activation
        # and writes gelu' (into a scratch buffer), where the plain no-grad forward takes the fp32 pre-activation.  The chunked step's first
        # pass sets it (clibd_amd.chunked): its cached embeddings must be the bits the saving forward of pass 2 produces.
        self.train_arithmetic = False

    HEAD_DIMS = (64, 128, 192)
    DGRAD8_C2_EVERY = 64  # full fine-tune: refreshes (= steps) between two host reads of the fc2 images' l1 norms

    def set_numerics(self, **settings):
        before = (self.numerics.get("ln_fold"), self.numerics.get("dgrad"))
        self.numerics.update(check_numerics(settings))
        if (self.numerics.get("ln_fold"), self.numerics.get("dgrad")) != before:
            self._cache_key = None   # the fold's / the 8-bit dgrad's weight images are built with the frozen-weight images, only while the switch is on
            self._c2 = None

    def _dgrad8_ok(self) -> bool:
        """dgrad = "fp8" is on and this stack can take it (see NUMERICS_CHOICES); raises for a configuration that cannot."""
        if self.numerics["dgrad"] != "fp8":
            return False
        if self.numerics["residual_grad"] != "bf16":
            raise NotSupportedYet("dgrad=fp8 needs residual_grad=bf16")
        if self.H % 256 or self.H < 512 or self.FF % 256:
            raise NotSupportedYet("dgrad=fp8 needs hidden % 256 == 0, hidden >= 512, intermediate % 256 == 0")
        return True

    # ---- fp8-forward mode (BASELINE.json configs[4]) ----------------------------------------------------------------
    # activation sites, named by the GEMM that consumes them
    FP8_SITES = ("qkv_in", "proj_in", "fc1_in", "fc2_in")
    FP8_SCALES = dict(qkv_in=8.0, proj_in=32.0, fc1_in=8.0, fc2_in=4.0)

    def enable_fp8(self, scales: Optional[dict] = None, amax: Optional[list] = None, margin: float = 2.0, sites: Optional[Sequence[str]] = None):
        """The four forward GEMMs of every layer run on the fp8 MFMA (ops.gemm_fp8_nt): frozen weights are quantised per
        output channel once; activations per tensor, inside the kernels that produce them (LayerNorm, attention, fc1
        epilogue), as e4m3(value * scale) saturating at +-448.  Scales are powers of two, per layer and site:
          * amax = [{site: max |activation|} per layer] (from calibrate(): one bf16 forward over a representative batch):
            scale = 2^floor(log2(448 / (margin * amax)));
          * otherwise the static `scales` / FP8_SCALES for every layer (fits unit-variance LayerNorm outputs, random-init or
            lightly trained towers; pretrained checkpoints with outlier channels want the calibration).
        The backward is unchanged bf16 (it needs gelu', qkv, statistics and — for the adapters — the bf16 LayerNorm output
        only): gradients are those of the bf16 network evaluated at the fp8 forward's activations.
        sites (round 5): a subset of FP8_SITES — ("fc1_in", "fc2_in") runs the MLP of every block on the fp8 MFMA
        and leaves QKV, attention and the projection on bf16 operands (the per-layer dicts then hold those sites only, which is also
        how the oracle is told: a site without a scale is a bf16 site).  The oracle study behind it: profiles/r05_exp_fp8_vit_sites.log.
        Trainable base weights (full fine-tune, full_mode()): the MLP-pair selection only.  The weight gradients of fc1 and fc2 contract
        the e4m3 operands the forward GEMMs consumed, dW = dY^T . e4m3(x sa) / sa (ops.gemm_tn_splitk with an e4m3 b: exact upcast, the
        power-of-two 1 / sa in the fp32 epilogue), so the rule above holds for them too; the e4m3 weight images are re-made from the
        fp32 masters at every refresh (every step under full fine-tune).  The all-site selection stays LoRA / frozen-base only
        (embedding-grade)."""
        if sites is not None:
            sites = tuple(sites)
            if any(s not in self.FP8_SITES for s in sites):
                raise ValueError(f"enable_fp8: sites must come from {self.FP8_SITES}")
            if set(sites) != set(self.FP8_SITES):
                if set(sites) != {"fc1_in", "fc2_in"}:
                    raise NotSupportedYet("fp8 site selection: only the MLP pair (fc1_in, fc2_in) is built")
        if self.full_mode() and (sites is None or set(sites) != {"fc1_in", "fc2_in"}):
            raise NotSupportedYet("fp8 forward on every site needs frozen base weights (their gradients would need the bf16 GEMM inputs); "
                                  "with trainable base weights the MLP-pair selection (sites=('fc1_in', 'fc2_in')) is built")
        if self.H % 256 or self.H < 512 or self.FF % 256:
            raise NotSupportedYet("fp8 forward needs hidden % 256 == 0, hidden >= 512, intermediate % 256 == 0")
        base = dict(self.FP8_SCALES, **(scales or {}))
        if sites is not None:
            base = {k: v for k, v in base.items() if k in sites}
        per_layer = []
        for i in range(len(self.layers)):
            d = dict(base)
            if amax is not None:
                for site, v in amax[i].items():
                    if site not in d:
                        continue
                    v = float(v)
                    if v > 0.0 and math.isfinite(v):
                        d[site] = 2.0 ** math.floor(math.log2(448.0 / (margin * v)))
            per_layer.append(d)
        self.fp8 = per_layer
        self._cache_key = None

    def disable_fp8(self):
        self.fp8 = None
        self._cache_key = None

    def calibrate(self, on: bool = True):
        """on: the next bf16 forward records max |activation| per layer and fp8 site (device scalars, no sync);
        off: returns them as [{site: float}] and stops recording."""
        if on:
            self._calib = []
            return None
        rec, self._calib = self._calib, None
        return [{k: float(v) for k, v in d.items()} for d in (rec or [])]

    # ---- frozen-weight images ---------------------------------------------------------------------------------
    def _key(self):
        k = 0
        for L in self.layers:
            for p in L.frozen():
                k += p._version + (p.data_ptr() & 0xFFFF)
        return (k, self.layers[0].proj_w.device)

    def full_mode(self) -> bool:
        """True when any base (non-adapter) weight of the stack is trainable: model_config.disable_lora.
        The forward then keeps the extra GEMM inputs the weight gradients need and the backward runs down to layer 0."""
        return any(p.requires_grad for L in self.layers for p in L.frozen())

    def base_params(self):
        return [p for L in self.layers for p in L.frozen()]

    def refresh(self):
        key = self._key()
        if key == self._cache_key and not self.full_mode():  # the fused optimizer updates weights in place (no version bump)
            return
        self._cache = []
        with torch.no_grad():
            for L in self.layers:
                c = _LayerCache()
                wqkv = _f32c(L.qkv_w[0]) if len(L.qkv_w) == 1 else torch.cat([_f32c(w) for w in L.qkv_w], dim=0)
                c.wqkv, c.wqkv_t = ops.cast_bf16(wqkv), ops.cast_transpose_bf16(wqkv)
                c.bqkv = _f32c(L.qkv_b[0]).clone() if len(L.qkv_b) == 1 else torch.cat([_f32c(b) for b in L.qkv_b], dim=0)
                c.wo, c.wo_t, c.bo = ops.cast_bf16(_f32c(L.proj_w)), ops.cast_transpose_bf16(_f32c(L.proj_w)), _f32c(L.proj_b)
                c.w1, c.w1_t, c.b1 = ops.cast_bf16(_f32c(L.fc1_w)), ops.cast_transpose_bf16(_f32c(L.fc1_w)), _f32c(L.fc1_b)
                c.w2, c.w2_t, c.b2 = ops.cast_bf16(_f32c(L.fc2_w)), ops.cast_transpose_bf16(_f32c(L.fc2_w)), _f32c(L.fc2_b)
                c.g1, c.be1, c.g2, c.be2 = _f32c(L.ln1_w), _f32c(L.ln1_b), _f32c(L.ln2_w), _f32c(L.ln2_b)
                if self.fp8 is not None:
                    f8 = self.fp8[len(self._cache)]
                    if "qkv_in" in f8:   # (a site selection leaves the other sites' images unbuilt)
                        c.wqkv8, c.cs_qkv = ops.quantize_rows_fp8(wqkv.contiguous(), f8["qkv_in"])
                        c.wo8, c.cs_o = ops.quantize_rows_fp8(_f32c(L.proj_w), f8["proj_in"])
                    c.w18, c.cs_1 = ops.quantize_rows_fp8(_f32c(L.fc1_w), f8["fc1_in"])
                    c.w28, c.cs_2 = ops.quantize_rows_fp8(_f32c(L.fc2_w), f8["fc2_in"])
                c.w1g = c.s1 = c.b1f = None
                if self.pre_ln and self.numerics["ln_fold"] == "on" and not self.full_mode():   # operand image of the norm2 -> fc1 fold, once per weight version
                    c.w1g, c.s1, c.b1f = ops.ln_fold_weights(_f32c(L.fc1_w), c.g2, c.be2, c.b1)
                c.v_fwd = c.v_bwd = c.a_cat = c.w_dt = c.slot2 = None
                c.wo_t8 = c.cs_ot = c.w1_t8 = c.cs_1t = c.w2_t8 = c.cs_2t = c.c2 = None
                self._cache.append(c)
            if self._dgrad8_ok():   # e4m3 images of the transposed weights, once per weight version
                # Full fine-tune (round 6): the weights move every step, so the images are re-quantised every step with the bf16 images they
                # are made from.  The per-layer constant c2 needs the l1 norm on the HOST (a kernel argument): it is re-derived every
                # DGRAD8_C2_EVERY refreshes only, and carries one binade of headroom (c2 / 2) for the growth of l1max in between.
                dev = self._cache[0].w2_t.device
                full = self.full_mode()
                reuse = full and self._c2 is not None and len(self._c2) == len(self._cache) and self._c2_age < self.DGRAD8_C2_EVERY
                l1 = None if reuse else torch.zeros((len(self._cache),), dtype=F32, device=dev)
                for i, c in enumerate(self._cache):
                    c.w2_t8, c.cs_2t = ops.quantize_rows_fp8_bf16(c.w2_t, 1.0, None if reuse else l1[i:i + 1])
                    c.wo_t8, c.cs_ot = ops.quantize_rows_fp8_bf16(c.wo_t, 1.0)
                if reuse:
                    self._c2_age += 1
                else:
                    # d(fc1 out) = e4m3(acc * col_scale * gelu' * c2): |acc * col_scale| <= 256 * l1max (scaled row maxima < 256), |gelu'| <= 1.13
                    self._c2 = [2.0 ** (math.floor(math.log2(448.0 / (256.0 * 1.13 * max(v, 1e-30)))) - (1 if full else 0))
                                for v in l1.cpu().tolist()]   # (one synchronisation per weight version; per DGRAD8_C2_EVERY steps under full fine-tune)
                    self._c2_age = 1
                for c, c2 in zip(self._cache, self._c2):
                    c.c2 = c2
                    c.w1_t8, c.cs_1t = ops.quantize_rows_fp8_bf16(c.w1_t, c.c2)   # its col_scale carries 1 / c2
        self._cache_key = key

    def pack_lora(self):
        """Per step: adapter parameters are trainable, so their bf16 operand images are rebuilt."""
        H = self.H
        for L, c in zip(self.layers, self._cache):
            if L.lora is None:
                continue
            dev = L.proj_w.device
            images = lambda: dict(v_fwd=torch.empty((3 * H, 8), dtype=BF16, device=dev), v_bwd=torch.empty((H, 8), dtype=BF16, device=dev),
                                  a_cat=torch.empty((8, H), dtype=BF16, device=dev), w_dt=torch.empty((16, 3 * H), dtype=BF16, device=dev))
            if c.v_fwd is None:
                im = images()
                c.v_fwd, c.v_bwd, c.a_cat, c.w_dt = im["v_fwd"], im["v_bwd"], im["a_cat"], im["w_dt"]
            slots = _rank_slots(L.lora)
            ops.lora_pack(*slots[0], c.v_fwd, c.v_bwd, c.a_cat, c.w_dt)
            if len(slots) > 1:      # ranks above 4: one more rank-(4+4) slot per four ranks (c.slot2: the list of their operand images)
                if self.fp8 is not None:
                    raise NotSupportedYet("fp8 forward with LoRA rank > 4")
                if c.slot2 is None or len(c.slot2) != len(slots) - 1:
                    c.slot2 = [images() for _ in slots[1:]]
                for sl, im in zip(slots[1:], c.slot2):
                    ops.lora_pack(*sl, im["v_fwd"], im["v_bwd"], im["a_cat"], im["w_dt"])
            else:
                c.slot2 = None

    # ---- further rank slots (r > 4): a pass each, built from the existing kernels — a zero-operand GEMM whose rank-8 MFMA step
    # carries u . V^T into an fp32 addend, which the layer's real GEMM then takes as its fp32 residual: ONE rounding of the sum,
    # as in the reference's B(A x) over all r columns
    def _slot2_addend(self, u, v, N, residual=None):
        M = u.shape[0]
        out = torch.empty((M, N), dtype=F32, device=u.device)
        ops.gemm_nt(torch.zeros((M, 64), dtype=BF16, device=u.device), torch.zeros((N, 64), dtype=BF16, device=u.device), rank_u=u, rank_v=v,
                    residual=residual, out_f32=out)
        return out

    def _slot2_fwd(self, c, x_bf16):
        """(fp32 [M,3H] addend sum_j (x A_j^T) B_j^T over the slots j >= 1 on the q and v columns, [t_j]): the slots chain through the
        addend (each zero-operand GEMM takes the previous sum as its fp32 residual), so the layer's GEMM still rounds the whole sum once."""
        add32, ts = None, []
        if c.slot2 is None:
            return None, None
        for im in c.slot2:
            tj = ops.lora_down_proj(x_bf16, im["a_cat"])
            add32 = self._slot2_addend(tj, im["v_fwd"], 3 * self.H, residual=add32)
            ts.append(tj)
        return add32, ts

    def _slot2_bwd_addend(self, c, dt2, residual=None):
        """fp32 [M,H] sum_j dt_j . A_cat_j over the slots j >= 1 (+ residual): joins the QKV dgrad as its fp32 addend."""
        add32 = residual
        for im, dtj in zip(c.slot2, dt2):
            add32 = self._slot2_addend(dtj, im["v_bwd"], self.H, residual=add32)
        return add32

    def lora_a(self, i: int):
        if i >= len(self.layers) or self.layers[i].lora is None:
            return None
        return self._cache[i].a_cat

    # ---- forward ------------------------------------------------------------------------------------------------
    # A layer is a short sequence of shared steps — qkv, attend, proj, mlp — between its two LayerNorms; every kernel role has ONE call
    # site below.  The steps take the layer's weight images `c`, the per-call plan `p`, the layer's fp8 scales (None = the
    # bf16 form) and their operand buffers; they keep no buffer (what one allocates it hands back), so the layer code owns every lifetime.
    def _qkv_fwd(self, c, fa, x, x8, ru, add32, qkv):
        """qkv = x Wqkv^T + b + ru . V^T (rank-8 LoRA step; + add32, the further rank slots' fp32 addend): e4m3 (x8) or bf16 (x) operands"""
        rv = c.v_fwd if ru is not None else None
        if fa is not None:
            ops.gemm_fp8_nt(x8, c.wqkv8, c.cs_qkv, bias=c.bqkv, rank_u=ru, rank_v=rv, out_bf16=qkv)
        else:
            ops.gemm_nt(x, c.wqkv, bias=c.bqkv, rank_u=ru, rank_v=rv, residual=add32, out_bf16=qkv)

    def _attend(self, p, fa, qkv, o, drop=None):
        """full-sequence attention into o (e4m3 with the projection's scale under the all-site fp8 forward).  Returns (o, att_sv): the
        training forward of the single-pass attention backward writes this layer's own o and saves its rounding residual and the lse."""
        o_lo = lse = None
        if self.dh != 64:   # wide heads: the training forward saves the lse its backward starts from; the no-grad forward passes none
            if p.save:
                lse = torch.empty((p.B * self.heads * p.S,), dtype=F32, device=p.dev)
            ops.attention_wide_fwd(qkv, p.B, p.S, self.heads, self.dh, o, lse=lse, drop=drop)
            return o, (dict(lse=lse) if p.save else None)
        if p.sp_ok:
            o = o if p.keep else p.new(self.H, BF16)
            o_lo, lse = p.new(self.H, BF16), torch.empty((p.B * self.heads * p.S,), dtype=F32, device=p.dev)
        ops.attention_fwd(qkv, p.B, p.S, self.heads, p.key_mask, o, drop=drop, out_fp8_scale=fa["proj_in"] if fa is not None else 0.0,
                          lse=lse, o_lo=o_lo)
        return o, (dict(o_att=o, o_lo=o_lo, lse=lse) if p.sp_ok else None)

    def _proj_fwd(self, p, c, fa, o, res, out, drop=None, fold_to=None):
        """out = [dropout](o Wo^T + b) + res (fp32).  fold_to = (x bf16, stats): the producer of the norm2 -> fc1 fold — the LayerNorm never
        makes a pass of its own: the projection also writes bf16(out) and its row sums, a small kernel turns those into (mean, rstd) —
        what the LayerNorm backward reads — and fc1 applies them to (x . (gamma o W1)^T) in its epilogue (_mlp_fwd)."""
        if fa is not None:
            ops.gemm_fp8_nt(o, c.wo8, c.cs_o, bias=c.bo, residual=res, out_f32=out, drop=drop)
            return
        xb, st = fold_to if fold_to is not None else (None, None)
        ops.gemm_nt(o, c.wo, bias=c.bo, residual=res, out_f32=out, drop=drop, out_bf16=xb,
                    row_sums=p.fold_sums if xb is not None else None)
        if xb is not None:
            ops.rowsum_finalize(p.fold_sums, self.eps, st)

    def _mlp_fwd(self, p, c, f8, x, res, out, h, a, drop=None, fold_st=None):
        """a = gelu(x W1^T + b1) with gelu' saved into h (all the backward needs); out = [dropout](a W2^T + b2) + res.  The fp8 fc1 and the
        fold's consumer epilogue (fold_st = the row statistics) always write gelu': into the scratch buffer when nothing is saved."""
        if f8 is not None:
            ops.gemm_fp8_nt(x, c.w18, c.cs_1, bias=c.b1, gelu_out_fp8=a, gelu_out_scale=f8["fc2_in"],
                            out_pre=h if h is not None else p.h_tmp)
            ops.gemm_fp8_nt(a, c.w28, c.cs_2, bias=c.b2, residual=res, out_f32=out, drop=drop)
            return
        if fold_st is not None:
            w1, b1, act, pre = c.w1g, c.b1f, ops.ACT_GELU_SAVE_GRAD, h if h is not None else p.h_tmp
            kw = dict(row_stats=fold_st, col_sum_w=c.s1)
        else:
            if h is None and p.scratch_h is not None:
                h = p.new(*p.scratch_h, x.shape[0])   # train_arithmetic: gelu' goes to a scratch buffer nobody reads
            w1, b1, act, pre, kw = c.w1, c.b1, p.act_save if h is not None else ops.ACT_GELU, h, {}
        ops.gemm_nt(x, w1, bias=b1, act=act, out_pre=pre, out_bf16=a, **kw)
        ops.gemm_nt(a, c.w2, bias=c.b2, residual=res, out_f32=out, drop=drop)

    def forward(self, x_f32, x_bf16, t0, B: int, S: int, key_mask, save: bool, cls_only_last: bool = False, drop=None, full: bool = False,
                x_fp8=None):
        """x_f32 [M,H] residual stream entering layer 0.  Post-LN stacks also pass its bf16 image and the layer-0
        adapter down-projection t0 (both produced by the embedding LayerNorm).  Returns (x_f32, x_bf16, saved).
        cls_only_last (pre-LN only): the caller consumes token 0 only, so the LAST block evaluates attention for that
        query, and projection + MLP for that row, per sequence — the returned x_f32 is then [B,H] (the other rows of
        the last block are dead code the reference computes and discards).
        drop (post-LN only): (p_hidden, p_attention, base_seed) — HF BERT train-mode dropout; site seeds via ops.derive_seed.
        full: full fine-tune mode — every layer keeps its own attention output, MLP input and GELU output (the X operands of
        the weight gradients) instead of sharing temporaries; under the fp8 MLP-pair selection the MLP input and GELU output are the
        e4m3 images the fp8 GEMMs consumed, recorded with their scales (x_mlp_s, a_s).
        x_fp8 (post-LN, fp8-forward mode): the e4m3 image of x (scale fp8[0]["qkv_in"]) from the embedding LayerNorm."""
        H, FF, M = self.H, self.FF, B * S
        dev = x_f32.device
        new = lambda cols, dt, rows=M: torch.empty((rows, cols), dtype=dt, device=dev)
        keep = save and full
        f8s = self.fp8
        mode = None if f8s is None else ("all" if "qkv_in" in f8s[0] else "mlp")   # "mlp": QKV / attention / projection stay bf16
        if mode == "all" and full:
            raise NotSupportedYet("fp8 forward on every site with trainable base weights (the MLP-pair selection is built)")
        wide = self.dh != 64
        if wide and key_mask is not None:
            raise NotSupportedYet(f"a key mask with head_dim {self.dh}: the wide-head attention kernels take full sequences only (head_dim 64 has the masked form)")
        if wide and cls_only_last:
            raise NotSupportedYet(f"the class-row-only last block with head_dim {self.dh} (head_dim 64 only)")
        if wide and mode == "all":
            raise NotSupportedYet(f"fp8 forward on every site with head_dim {self.dh}: the wide-head attention writes no e4m3 output "
                                  "(the MLP-pair selection, sites=('fc1_in', 'fc2_in'), is built)")
        cal = self._calib if f8s is None else None      # calibration pass: bf16 forward recording max |operand| per site
        amax = lambda t_: t_.abs().amax().float()
        AT = ops.FP8 if f8s is not None else BF16    # dtype of the GEMM-operand temporaries
        o = None if keep else new(H, BF16 if mode == "mlp" else AT)   # attention output (temporary, reused by every layer)
        a = None if keep else new(FF, AT)           # post-GELU activation (temporary)
        xn2 = new(H, AT) if (self.pre_ln and not keep) else None
        xn8 = new(H, ops.FP8) if mode == "all" else None   # fp8 image of the first LayerNorm's output (temporary)
        # storage of gelu'(fc1 out): bf16 (default), one byte, or (round 6) the 12-bit e4m7 form of the bf16 value; the fp8-forward fc1
        # and the LN -> fc1 fold's consumer epilogue write bf16 only
        gg = self.numerics["gelu_grad"]
        if f8s is not None or (self.pre_ln and self.numerics["ln_fold"] == "on"):
            gg = "bf16"
        GG = BF16 if gg == "bf16" else torch.uint8
        HC = 3 * FF // 2 if gg == "e4m7" else FF                                                     # columns of that buffer
        act_save = {"bf16": ops.ACT_GELU_SAVE_GRAD, "u8": ops.ACT_GELU_SAVE_GRAD_U8, "e4m7": ops.ACT_GELU_SAVE_GRAD_E12}[gg]
        h_tmp = new(FF, BF16) if (f8s is not None and not save) else None       # the fp8 fc1 form always writes gelu'
        sp_ok = save and key_mask is None and f8s is None and S <= 224 and self.numerics["attn_bwd"] == "sp" and not wide
        # norm2 -> fc1 as the algebraic fold (numerics ln_fold): pre-LN, frozen base, bf16 forward, shapes the 256x256 kernel takes
        fold = (self.pre_ln and self.numerics["ln_fold"] == "on" and self._cache[0].w1g is not None and f8s is None and not full
                and GG == BF16 and H % 256 == 0 and FF % 256 == 0 and M >= 1024 and ((M + 255) // 256) * (H // 256) >= 128
                and H % 128 == 0)
        fold_sums = torch.empty((H // 128, M, 2), dtype=F32, device=dev) if fold else None
        if fold and h_tmp is None and not save:
            h_tmp = new(FF, BF16)   # the consumer epilogue always writes gelu' (eval forward: into a scratch buffer)
        p = SimpleNamespace(B=B, S=S, dev=dev, new=new, key_mask=key_mask, keep=keep, sp_ok=sp_ok, act_save=act_save, h_tmp=h_tmp,
                            fold_sums=fold_sums, save=save, scratch_h=(HC, GG) if (self.train_arithmetic and not save) else None)
        t, saved = t0, []
        for i, (L, c) in enumerate(zip(self.layers, self._cache)):
            lora = L.lora is not None
            f8 = f8s[i] if f8s is not None else None
            fa = f8 if mode == "all" else None     # the scales of the attention half: None = its bf16 form
            crec = {} if cal is not None else None
            rec = {}     # what the backward needs of this layer (filled under `save`)
            if keep:   # (fp8 MLP pair: the MLP's operands are the e4m3 images the weight gradients contract)
                o, a = new(H, BF16), new(FF, AT)
                xn2 = new(H, AT) if self.pre_ln else None
            if self.pre_ln and cls_only_last and i == len(self.layers) - 1:
                # LN1 and QKV over all rows (the full-size GEMM of this block, fp8 under the all-site mode); the class-row remainder
                # of the block stays bf16
                xn = new(H, BF16)
                st1 = new(2, F32)
                t = new(8, BF16) if lora else None
                qkv = new(3 * H, BF16)
                ops.layernorm_fwd(x_f32, c.g1, c.be1, self.eps, y_bf16=xn, stats=st1, lora_a=c.a_cat if lora else None, t_out=t,
                                  y_fp8=xn8, fp8_scale=fa["qkv_in"] if fa is not None else 0.0)
                add32, t2 = self._slot2_fwd(c, xn)
                self._qkv_fwd(c, fa, xn, xn8, t, add32, qkv)
                if crec is not None:
                    crec["qkv_in"] = amax(xn)
                o_cls = new(H, BF16, B)
                ops.attention_fwd(qkv, B, S, self.heads, key_mask, o_cls, nq=1)
                x_cls = ops.gather_rows(x_f32.view(B, S, H))
                x1 = new(H, F32, B)
                self._proj_fwd(p, c, None, o_cls, x_cls, x1)
                st2 = new(2, F32, B)
                xn2c = new(H, BF16, B)
                ops.layernorm_fwd(x1, c.g2, c.be2, self.eps, y_bf16=xn2c, stats=st2)
                h = new(HC, GG, B) if save else None
                ac = new(FF, BF16, B)
                x2 = new(H, F32, B)
                self._mlp_fwd(p, c, None, xn2c, x1, x2, h, ac)
                if save:
                    rec = dict(x_in=x_f32, st1=st1, x_qkv=xn, t=t, t2=t2, qkv=qkv, x1=x1, st2=st2, h=h, cls_only=True)
                if keep:
                    rec.update(o=o_cls, x_mlp=xn2c, a=ac)
                x_f32 = x2
            elif self.pre_ln:
                # xn = LN1(x) (+ t = xn·A^T);  qkv = xn Wqkv^T + b + t·B^T
                xn = new(H, BF16)
                st1 = new(2, F32)
                t = new(8, BF16) if lora else None
                qkv = new(3 * H, BF16)
                x1 = new(H, F32)
                st2 = new(2, F32)
                h = new(HC, GG) if save else None        # holds gelu'(fc1 out): all the backward needs
                x2 = new(H, F32)
                folded = fold and cal is None
                ops.layernorm_fwd(x_f32, c.g1, c.be1, self.eps, y_bf16=xn, stats=st1, lora_a=c.a_cat if lora else None, t_out=t,
                                  y_fp8=xn8, fp8_scale=fa["qkv_in"] if fa is not None else 0.0)
                add32, t2 = self._slot2_fwd(c, xn)
                self._qkv_fwd(c, fa, xn, xn8, t, add32, qkv)
                o, att_sv = self._attend(p, fa, qkv, o)
                self._proj_fwd(p, c, fa, o, x_f32, x1, fold_to=(xn2, st2) if folded else None)
                if not folded:
                    ops.layernorm_fwd(x1, c.g2, c.be2, self.eps, stats=st2,
                                      **(dict(y_bf16=xn2) if f8 is None else dict(y_fp8=xn2, fp8_scale=f8["fc1_in"])))
                self._mlp_fwd(p, c, f8, xn2, x1, x2, h, a, fold_st=st2 if folded else None)
                if crec is not None:
                    crec.update(qkv_in=amax(xn), proj_in=amax(o), fc1_in=amax(xn2), fc2_in=amax(a))
                if save:
                    rec = dict(x_in=x_f32, st1=st1, x_qkv=xn, t=t, t2=t2, qkv=qkv, x1=x1, st2=st2, h=h, **(att_sv or {}))
                if keep:
                    rec.update(o=o, x_mlp=xn2, a=a, **(dict(x_mlp_s=f8["fc1_in"], a_s=f8["fc2_in"]) if f8 is not None else {}))
                x_f32 = x2
            else:
                d_att = d_h1 = d_h2 = None
                if drop is not None:
                    p_h, p_a, base = drop
                    d_att = ops.Drop(p_a, ops.derive_seed(base, i, 0))
                    d_h1 = ops.Drop(p_h, ops.derive_seed(base, i, 1))
                    d_h2 = ops.Drop(p_h, ops.derive_seed(base, i, 2))
                qkv = new(3 * H, BF16)
                s1 = new(H, F32)
                x1_f32 = new(H, F32)
                st1 = new(2, F32)
                h = new(HC, GG) if save else None
                s2 = new(H, F32)
                x2_f32, x2_bf16 = new(H, F32), new(H, BF16)
                st2 = new(2, F32)
                nxt = self.lora_a(i + 1)
                t_next = new(8, BF16) if nxt is not None else None
                if fa is not None and x_fp8 is None:
                    raise ValueError("fp8 forward (post-LN): the caller passes the e4m3 image of x")
                # the MLP's input: LayerNorm 1 writes it as bf16, or as e4m3 under either fp8 mode (round 5: also on the MLP pair only)
                x_mlp = new(H, BF16) if f8 is None else (xn8 if fa is not None else new(H, ops.FP8))
                add32, t2 = self._slot2_fwd(c, x_bf16)
                self._qkv_fwd(c, fa, x_bf16, x_fp8, t if lora else None, add32, qkv)
                o, att_sv = self._attend(p, fa, qkv, o, drop=d_att)
                self._proj_fwd(p, c, fa, o, x_f32, s1, drop=d_h1)
                ops.layernorm_fwd(s1, c.g1, c.be1, self.eps, y_f32=x1_f32, stats=st1,
                                  **(dict(y_bf16=x_mlp) if f8 is None else dict(y_fp8=x_mlp, fp8_scale=f8["fc1_in"])))
                self._mlp_fwd(p, c, f8, x_mlp, x1_f32, s2, h, a, drop=d_h2)
                x8_next = new(H, ops.FP8) if fa is not None else None     # the next layer's QKV operand, at that layer's scale
                ops.layernorm_fwd(s2, c.g2, c.be2, self.eps, y_bf16=x2_bf16, y_f32=x2_f32, stats=st2, lora_a=nxt, t_out=t_next,
                                  y_fp8=x8_next, fp8_scale=f8s[min(i + 1, len(f8s) - 1)]["qkv_in"] if fa is not None else 0.0)
                if crec is not None:
                    crec.update(qkv_in=amax(x_bf16), proj_in=amax(o), fc1_in=amax(x_mlp), fc2_in=amax(a))
                if save:
                    rec = dict(x_qkv=x_bf16, t=t if lora else None, t2=t2, qkv=qkv, s1=s1, st1=st1, h=h, s2=s2, st2=st2,
                               d_att=d_att, d_h1=d_h1, d_h2=d_h2, **(att_sv or {}))
                if keep:
                    rec.update(o=o, x_mlp=x_mlp, a=a, **(dict(x_mlp_s=f8["fc1_in"], a_s=f8["fc2_in"]) if f8 is not None else {}))
                x_f32, x_bf16, t, x_fp8 = x2_f32, x2_bf16, t_next, x8_next
            saved.append(rec)
            if cal is not None:
                cal.append(crec)
        return x_f32, x_bf16, saved

    # ---- backward -----------------------------------------------------------------------------------------------
    def layer_params(self, i: int):
        """Every parameter of layer i a gradient can be produced for (base weights + adapters)."""
        L = self.layers[i]
        return L.frozen() + (L.lora.tensors() if L.lora is not None else [])

    # The backward's steps, mirror images of the forward's (mlp, proj, qkv and ONE LayerNorm-backward helper), take the layer's parameter
    # handles L, its weight images c, its saved record and the per-call plan p.  A gradient operand is a bf16 matrix `dy` and, under the
    # 8-bit dgrad, also `dy8` = (e4m3 rows, one dequantisation factor per row) as the LayerNorm backward before it wrote them.
    def _wgrad(self, p, dy, x, ws, bs, xs=None):
        """full fine-tune: weight / bias gradients of one Linear (fp8 forward, MLP pair: x is the e4m3 GEMM input, xs its scale)"""
        if p.full:
            linear_wgrad(dy, x, ws, bs, p.grads, x_scale=xs, **_ordered(p.det))

    def _ln_bwd(self, p, dy, x, st, gamma, w, b, *, dres=None, f32=False, bf16=False, res16=False, q8=False, drop=None):
        """One LayerNorm backward: dx = LN'(dy) [+ dres, fp32 or bf16 by its dtype], written in each requested form.  Returns
        (dx_f32, dx_bf16, dx_res_bf16, dx8): fp32; bf16 (carrying the dropout mask of `drop`); the un-dropped bf16 residual copy of the
        post-LN bf16 stream; the (e4m3 rows, row dequantisation factors) pair the 8-bit dgrad GEMMs take.  Full fine-tune: d(gamma) and
        d(beta) accumulate in the same pass (the kernel holds dy and xhat anyway)."""
        mk = lambda dt: torch.empty(x.shape, dtype=dt, device=x.device)
        # (allocated in the order these forms always were: the caching allocator's block reuse, and the peak it reports, follow it)
        dx_f32 = mk(F32) if f32 else None
        dx_bf16 = mk(BF16) if bf16 and not res16 else None
        dx_res = mk(BF16) if res16 else None
        dx8 = (mk(torch.uint8).view(ops.FP8), torch.empty((x.shape[0],), dtype=F32, device=x.device)) if q8 else None
        if bf16 and res16:
            dx_bf16 = mk(BF16)
        kw = {} if dres is None else {"dres" if dres.dtype == F32 else "dres_bf16": dres}
        if q8:
            kw.update(dx_fp8=dx8[0], row_dequant=dx8[1])
        if p.full:
            kw.update(ln_param_grads(p.grads, w, b, p.det))
        ops.layernorm_bwd(dy, x, st, gamma, dx_f32=dx_f32, dx_bf16=dx_bf16, dx_res_bf16=dx_res, drop=drop, **kw)
        return dx_f32, dx_bf16, dx_res, dx8

    def _mlp_bwd(self, p, L, c, rec, dy, dy8, out, dh=None, **join):
        """fc2 weight gradient; d(fc1 out) = (dy W2) o gelu' -> dh; fc1 weight gradient; out = dh W1 with the ONE epilogue that joins the
        stream (`join`): none, act=ACT_ADD_AUX + aux (bf16 stream) or residual (fp32 stream, fp32 out).  dy8: both dgrads on e4m3 operands
        — d(fc1 out) leaves as e4m3 with the rows' scales x c2, the fc1 dgrad divides both back out; under full fine-tune the fc2 dgrad
        writes it once more as bf16, the operand of fc1's weight gradient.  dh: the caller's buffer (class rows) or the walk's."""
        h = rec["h"]
        self._wgrad(p, dy, rec.get("a"), [L.fc2_w], [L.fc2_b], rec.get("a_s"))
        if dy8 is not None:
            p.dh8 = p.new(self.FF, torch.uint8).view(ops.FP8)
        if dh is None and (dy8 is None or p.full):
            dh = p.dh = p.new(self.FF, BF16) if p.dh is None else p.dh
        if dy8 is not None:
            ops.gemm_fp8_dgrad_nt(dy8[0], c.w2_t8, c.cs_2t, aux=h, act=_mul_aux_act(h, self.FF), out_fp8=p.dh8, out_fp8_scale=c.c2,
                                  a_row_dequant=dy8[1] if p.full else None, out_bf16_dual=dh if p.full else None)
        else:
            ops.gemm_nt(dy, c.w2_t, act=_mul_aux_act(h, self.FF), aux=h, out_bf16=dh)
        self._wgrad(p, dh, rec.get("x_mlp"), [L.fc1_w], [L.fc1_b], rec.get("x_mlp_s"))
        if dy8 is not None:
            ops.gemm_fp8_dgrad_nt(p.dh8, c.w1_t8, c.cs_1t, a_row_dequant=dy8[1], out_bf16=out, **join)
        else:
            ops.gemm_nt(dh, c.w1_t, **{"out_f32" if out.dtype == F32 else "out_bf16": out}, **join)

    def _proj_bwd(self, p, L, c, rec, dy, dy8, out):
        """projection weight gradient; out = d(attention out) = dy Wo (bf16)"""
        self._wgrad(p, dy, rec.get("o"), [L.proj_w], [L.proj_b])
        if dy8 is not None:
            ops.gemm_fp8_dgrad_nt(dy8[0], c.wo_t8, c.cs_ot, a_row_dequant=dy8[1], out_bf16=out)
        else:
            ops.gemm_nt(dy, c.wo_t, out_bf16=out)

    def _qkv_bwd(self, p, L, c, rec, dqkv, dt, out=None, new_out=None, residual=None, **join):
        """adapter gradients (+ dt, the rank-8 operand of the dgrad), QKV weight gradient, then — unless nothing trainable lies below
        (neither `out` nor `new_out`) — the QKV dgrad dqkv Wqkv + dt . V^T [+ the further rank slots' fp32 addend] with the epilogue
        that joins the stream, into `out` or a fresh [M,H] matrix of dtype `new_out`; returns it."""
        lora = L.lora is not None
        dt2 = self._lora_grads(L, c, dqkv, rec["x_qkv"], rec["t"], dt, p.grads, rec.get("t2")) if lora else None
        self._wgrad(p, dqkv, rec["x_qkv"], L.qkv_w, L.qkv_b)
        if out is None and new_out is None:
            return None
        # further rank slots: sum_j dt_j . A_cat_j, fp32 (held on the plan until the next layer's replaces it)
        add32 = p.add32 = residual if dt2 is None else self._slot2_bwd_addend(c, dt2, residual=residual)
        out = p.new(self.H, new_out) if out is None else out
        ops.gemm_nt(dqkv, c.wqkv_t, rank_u=dt if lora else None, rank_v=c.v_bwd if lora else None, residual=add32,
                    **{"out_f32" if out.dtype == F32 else "out_bf16": out}, **join)
        return out

    def backward(self, dx_f32, dx_bf16, saved, B: int, S: int, key_mask, grads: dict, full: bool = False, on_layer_done=None):
        """dx = gradient w.r.t. the stack output (fp32 residual stream; pre-LN also needs its bf16 image).
        on_layer_done(i): called once layer i's parameter gradients are complete (enqueued on the current stream) — the
        trainer's hook for starting that layer's gradient all-reduce under the rest of the backward.
        Fills grads[id(param)] for the adapters — and, in full fine-tune mode, for every base weight / bias / LayerNorm
        parameter present in `grads`; returns the fp32 gradient w.r.t. the stack input then (None in LoRA mode, where the
        walk stops at the lowest adapted layer because nothing below it is trainable)."""
        H, FF, M = self.H, self.FF, B * S
        dev = dx_f32.device
        new = lambda cols, dt, rows=M: torch.empty((rows, cols), dtype=dt, device=dev)
        dtmp = new(H, BF16)
        dqkv = new(3 * H, BF16)
        dt = new(16, BF16)
        first_lora = min((i for i, L in enumerate(self.layers) if L.lora is not None), default=len(self.layers))
        if full:
            first_lora = -1  # every layer has trainable parameters and the input gradient is needed
        # bf16 residual-gradient stream (see NUMERICS_CHOICES).  Round 4: full fine-tune mode takes it too — the LayerNorm parameter
        # gradients ride along in the same kernel (clibd_layernorm_bwd with dgamma / dbeta), and the BOTTOM layer hands an fp32 gradient to
        # the embedding backward as before.  409.6 ms per step at b = 2048 with the fp32 stream (profiles/r04_fullft_*_v1*).
        r16 = self.numerics["residual_grad"] == "bf16"
        # 8-bit dgrad (numerics dgrad = "fp8"): the LayerNorm backwards below also write their output as e4m3 rows + one dequantisation
        # factor per row, which the next dgrad GEMM takes as its A operand; dx8 = that pair for the incoming stream gradient.
        # Round 6: also with trainable base weights (full fine-tune, the reference's final recipe: `disable_lora: true`) — the dgrad takes
        # the e4m3 rows, every weight gradient stays bf16 (the LayerNorm backward then writes both copies, and the fc2 dgrad writes
        # d(fc1 out) twice: e4m3 for the fc1 dgrad, bf16 for the fc1 weight gradient).
        dg8 = (self._dgrad8_ok() and self._cache[0].w2_t8 is not None and M % 4 == 0
               and M * FF < 2 ** 32)   # (the fp8 kernel addresses operands with 32-bit byte offsets)
        q8_mlp, q8_proj = dg8 and "mlp" in self.dgrad8_sites, dg8 and "proj" in self.dgrad8_sites   # (pre-LN: per-site selection)
        dx8 = None
        # dh = d(fc1 out), bf16 [M,FF]: allocated by the first layer that takes the bf16 dgrad; dh8 = its e4m3 form, per layer
        p = SimpleNamespace(dev=dev, new=new, grads=grads, full=full, det=self.deterministic, dh=None, dh8=None, add32=None)
        # post-LN: `dx_f32` holds the incoming gradient of the layer output (fp32 from the head at the top layer; below it bf16 on the bf16
        # stream).  bf16 stream: each LayerNorm backward writes the un-dropped residual copy (res) and, under dropout, the masked copy
        # the dense branch consumes — not at all where the dgrad takes the e4m3 rows and no weight gradient wants it — and the two dgrads
        # that re-join the stream add the residual copy in their epilogue (ACT_ADD_AUX).  fp32 stream: the LayerNorm backward writes
        # fp32 + (masked) bf16 and the joining dgrads take the fp32 copy as their residual.
        dropped = lambda d: d is not None and d.thr16 > 0
        ln = lambda dy, x, st, g, w, b, d: self._ln_bwd(p, dy, x, st, g, w, b, drop=d, **(
            dict(res16=True, bf16=dropped(d) and (full or not dg8), q8=dg8) if r16 else dict(f32=True, bf16=True)))
        join = lambda f32, res: dict(act=ops.ACT_ADD_AUX, aux=res) if r16 else dict(residual=f32)
        for i in range(len(self.layers) - 1, -1, -1):
            L, c, rec = self.layers[i], self._cache[i], saved[i]
            if i < first_lora:
                break  # nothing trainable at or below this layer
            down = i > first_lora     # something trainable lies below: the gradient of this layer's input is needed
            if self.pre_ln:
                need32 = not r16 or (full and i == 0)
                if rec.get("cls_only"):
                    # dx_f32 / dx_bf16 are [B,H]: the gradient of the class-token row of this block's output
                    dhc, dtc = new(FF, BF16, B), new(H, BF16, B)
                    self._mlp_bwd(p, L, c, rec, dx_bf16, None, dtc, dh=dhc)
                    dx1_f32, dx1_bf16, _, _ = self._ln_bwd(p, dtc, rec["x1"], rec["st2"], c.g2, L.ln2_w, L.ln2_b, dres=dx_f32,
                                                           f32=True, bf16=True)
                    self._proj_bwd(p, L, c, rec, dx1_bf16, None, dtc)                                    # d(attn out), class rows
                    self._attention_bwd(rec, dtc, B, S, key_mask, dqkv, nq=1)
                else:
                    self._mlp_bwd(p, L, c, rec, dx_bf16, dx8, dtmp)                                      # d(LN2 out)
                    dx1_f32, dx1_bf16, _, dx18 = self._ln_bwd(p, dtmp, rec["x1"], rec["st2"], c.g2, L.ln2_w, L.ln2_b,
                                                              dres=dx_bf16 if r16 else dx_f32, f32=not r16, bf16=True, q8=q8_proj)
                    self._proj_bwd(p, L, c, rec, dx1_bf16, dx18, dtmp)                                   # d(attn out)
                    self._attention_bwd(rec, dtmp, B, S, key_mask, dqkv)
                self._qkv_bwd(p, L, c, rec, dqkv, dt, out=dtmp if down else None)
                if down:
                    if rec.get("cls_only"):   # residual path: class rows only (never rebound: this matrix lives to the end of the walk)
                        dres_cls = ops.scatter_rows(dx1_f32, S, bf16=r16, f32=not r16)[0 if r16 else 1]
                    dres = dres_cls if rec.get("cls_only") else (dx1_bf16 if r16 else dx1_f32)
                    dx_f32, dx_bf16, _, dx8 = self._ln_bwd(p, dtmp, rec["x_in"], rec["st1"], c.g1, L.ln1_w, L.ln1_b, dres=dres,
                                                           f32=need32, bf16=True, q8=q8_mlp)
            else:
                ds2_f32, ds2_b, ds2_res, ds2_8 = ln(dx_f32, rec["s2"], rec["st2"], c.g2, L.ln2_w, L.ln2_b, rec["d_h2"])
                dx1 = new(H, BF16 if r16 else F32)
                self._mlp_bwd(p, L, c, rec, ds2_b if ds2_b is not None else ds2_res, ds2_8, dx1, **join(ds2_f32, ds2_res))
                ds1_f32, ds1_b, ds1_res, ds1_8 = ln(dx1, rec["s1"], rec["st1"], c.g1, L.ln1_w, L.ln1_b, rec["d_h1"])
                self._proj_bwd(p, L, c, rec, ds1_b if ds1_b is not None else ds1_res, ds1_8, dtmp)
                self._attention_bwd(rec, dtmp, B, S, key_mask, dqkv, drop=rec["d_att"])
                # (bf16 stream, bottom layer of a full fine-tune: the embedding backward takes an fp32 gradient)
                ndx = self._qkv_bwd(p, L, c, rec, dqkv, dt, new_out=(F32 if not r16 or (full and i == 0) else BF16) if down else None,
                                    **join(ds1_f32, ds1_res))
                if down:
                    dx_f32 = ndx
            if on_layer_done is not None:
                on_layer_done(i)
        return dx_f32 if full else None

    def _attention_bwd(self, rec, dout, B, S, key_mask, dqkv, drop=None, nq=None):
        if self.dh != 64:   # wide heads: one backward form, from the forward's lse (no key mask, every query row: forward() refused the rest)
            ops.attention_wide_bwd(rec["qkv"], dout, rec["lse"], B, S, self.heads, self.dh, dqkv, drop=drop)
        elif "lse" in rec:   # the forward saved what the single-pass kernel needs
            ops.attention_bwd_sp(rec["qkv"], dout, rec["o_att"], rec["o_lo"], rec["lse"], B, S, self.heads, dqkv, drop=drop)
        else:
            ops.attention_bwd(rec["qkv"], dout, B, S, self.heads, key_mask, dqkv, nq=nq, drop=drop)

    def _lora_grads(self, L, c, dqkv, x_bf16, t, dt, grads, t2=None):
        """dt[:, 0:4] = dq·B_q, dt[:, 4:8] = dv·B_v (the rank-8 operand of the QKV dgrad that follows) and the four adapter gradients
        in one call: dq and dv are streamed once for dt and dB together (clibd_lora_backward); the k segment of dqkv is never read.
        Ranks other than 4 run on rank-4 slots (_rank_slots): scratch gradients, sliced back; ranks above 4 take one more call per slot
        with that slot's images and down-projection t2[j], whose dt (returned as a list) join the QKV dgrad as an fp32 addend (_slot2_bwd_addend)."""
        H = self.H
        lp = L.lora
        r = lp.a_q.shape[0]
        if r == 4:
            ops.lora_backward(dqkv, x_bf16, t, c.w_dt, dt, grads[id(lp.a_q)], grads[id(lp.a_v)], grads[id(lp.b_q)], grads[id(lp.b_v)], **_ordered(self.deterministic))
            return None
        dev = dqkv.device
        dt2 = []
        nslots = (r + 3) // 4
        for k in range(nslots):
            lo = 4 * k
            if k == 0:
                tk, w_dt, dtk = t, c.w_dt, dt
            else:
                tk, w_dt, dtk = t2[k - 1], c.slot2[k - 1]["w_dt"], torch.empty_like(dt)
                dt2.append(dtk)
            ga_q, ga_v = torch.zeros((4, H), dtype=F32, device=dev), torch.zeros((4, H), dtype=F32, device=dev)
            gb_q, gb_v = torch.zeros((H, 4), dtype=F32, device=dev), torch.zeros((H, 4), dtype=F32, device=dev)
            ops.lora_backward(dqkv, x_bf16, tk, w_dt, dtk, ga_q, ga_v, gb_q, gb_v, **_ordered(self.deterministic))
            n = min(4, r - lo)   # the padded rows / columns receive exact zeros' worth of signal
            grads[id(lp.a_q)][lo:lo + n].add_(ga_q[:n]); grads[id(lp.a_v)][lo:lo + n].add_(ga_v[:n])
            grads[id(lp.b_q)][:, lo:lo + n].add_(gb_q[:, :n]); grads[id(lp.b_v)][:, lo:lo + n].add_(gb_v[:, :n])
        dt2 = dt2 or None
        return dt2


def linear_wgrad(dy_bf16: torch.Tensor, x_bf16: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], grads: dict,
                 ordered: bool = False, x_scale: Optional[float] = None):
    """Weight / bias gradients of y = x W^T + b for the parameters present in `grads` (accumulating):
    dW [N,K] += dy^T x — read in place by the rows-contracting kernel when the shape allows (M % 128 == 0, N and K % 256 == 0:
    every full-size layer), else as the NT GEMM (dy^T [N,Mp]) (x^T [K,Mp])^T over zero-padded transposes —
    db += column sums of dy.  `weights` may be the row-wise pieces of a fused projection (BERT query / key / value).
    ordered (deterministic mode): every sum in a fixed order — the TN form's bias sums per slice, the generic GEMM unsplit (its split-K form
    accumulates atomically), the column-sum kernel through partials.
    x as float8_e4m3fn (fp8 forward): the GEMM input as the forward consumed it, e4m3(x * x_scale); dW += dy^T (x8 / x_scale) — the
    rows-contracting kernel's e4m3 form, or the transpose + NT path over a dequantising transpose (both exact upcasts)."""
    if not any(id(w) in grads for w in weights) and not any(id(b) in grads for b in biases):
        return
    if x_bf16 is None:
        raise RuntimeError("full fine-tune backward needs the layer's GEMM input (forward ran without full=True)")
    x8 = x_bf16.dtype == ops.FP8
    if x8 and (x_scale is None or not x_scale > 0.0):
        raise ValueError("linear_wgrad: an e4m3 input needs its quantisation scale (x_scale > 0)")
    tn_kw = dict(b_scale=1.0 / x_scale) if x8 else {}
    M = dy_bf16.shape[0]
    want_b = [b is not None and id(b) in grads for b in biases]
    bias_done = False
    K = x_bf16.shape[1]
    tn_ok = (M % 128 == 0 and M >= 256 and K % 256 == 0 and dy_bf16.stride(0) % 8 == 0 and x_bf16.stride(0) % 8 == 0
             and all(w.shape[0] % 256 == 0 for w in weights))
    pending = [id(w) in grads for w in weights]   # weight gradients still to be produced
    if tn_ok and any(pending):
        # in-place rows-contracting GEMM (gemm256_tn.hip): no dy^T / x^T; the bias gradient (column sums of dy) rides along.
        # A piece the kernel declines (ops.gemm_tn_splitk returns False) stays pending and takes the transpose path below.
        n0 = 0
        done = []
        for j, (w, b, wb) in enumerate(zip(weights, biases, want_b)):
            n1 = n0 + w.shape[0]
            took = False
            if pending[j]:
                cs = grads[id(b)].view(-1) if wb else None
                took = ops.gemm_tn_splitk(dy_bf16[:, n0:n1], x_bf16, grads[id(w)].view(w.shape[0], -1), accumulate=True, colsum=cs, **_ordered(ordered),
                                          **tn_kw)
                pending[j] = not took
            done.append(took and wb)
            n0 = n1
        want_b = [wb and not d for wb, d in zip(want_b, done)]   # biases whose weight is frozen still take the column-sum kernel
    if any(pending):
        N = dy_bf16.shape[1]
        csum, direct = None, False
        if any(want_b) and N % 8 == 0 and dy_bf16.stride(0) % 8 == 0:
            if len(weights) == 1:
                csum, direct = grads[id(biases[0])].view(-1), True        # one bias over all N columns: accumulate in place
            else:
                csum = torch.zeros((N,), dtype=F32, device=dy_bf16.device)   # column sums of dy in the same pass as its transpose
        dyT = ops.transpose_bf16(dy_bf16, pad_to=128, colsum=csum)   # [N, Mp]
        xT = ops.transpose_fp8(x_bf16, 1.0 / x_scale, pad_to=128) if x8 else ops.transpose_bf16(x_bf16, pad_to=128)     # [K, Mp]
        Mp = dyT.shape[1]
        split = 1 if ordered else max(1, min(32, Mp // 2048))
        n0 = 0
        for j, w in enumerate(weights):
            n1 = n0 + w.shape[0]
            if pending[j]:
                gw = grads[id(w)].view(w.shape[0], -1)
                if Mp >= 4096 and ops.gemm_nt_splitk(dyT[n0:n1], xT, gw, accumulate=True):
                    pass  # 256x256 kernel, one (tile, K-slice) per CU, partials summed by a second kernel
                elif split > 1:
                    ops.gemm_nt(dyT[n0:n1], xT, out_f32=gw, split_k=split)
                else:
                    ops.gemm_nt(dyT[n0:n1], xT, out_f32=gw, residual=gw)
            n0 = n1
        if csum is not None:
            n0 = 0
            for w, b, wb in zip(weights, biases, want_b):
                n1 = n0 + w.shape[0]
                if wb and not direct:
                    grads[id(b)].view(-1).add_(csum[n0:n1])
                n0 = n1
            bias_done = True
    if not bias_done:
        n0 = 0
        for w, b, wb in zip(weights, biases, want_b):
            n1 = n0 + w.shape[0]
            if wb:
                ops.colsum_bf16(dy_bf16[:, n0:n1], grads[id(b)], **_ordered(ordered))
            n0 = n1


class GradBucket:
    """One flat, zero-initialised fp32 buffer holding the gradients of a tower's trainable parameters."""

    def __init__(self, params: Sequence[torch.nn.Parameter]):
        self.params = list(params)
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros((max(n, 1),), dtype=F32, device=dev)
        self.views, off = {}, 0
        for p in self.params:
            self.views[id(p)] = self.flat[off : off + p.numel()].view(p.shape)
            off += p.numel()

    def ordered(self):
        return [self.views[id(p)] for p in self.params]


def dense_head_backward(dout_f32: torch.Tensor, x_bf16: torch.Tensor, weight: torch.nn.Parameter, bias: torch.nn.Parameter,
                        grads: dict, out_bf16: bool, ordered: bool = False):
    """y = x W^T + b with a TRAINABLE W [D,K]:  dW += dy^T x, db += colsum(dy), returns dx = dy W.
    dout_f32 [M,D] fp32 (M small: one row per sample) or bf16 [M,D].  ordered: fixed-order sums only (see linear_wgrad)."""
    dy_b = ops.cast_bf16(dout_f32) if dout_f32.dtype == F32 else dout_f32
    M, D = dy_b.shape
    K = x_bf16.shape[1]
    fused_bias = D % 8 == 0 and dy_b.stride(0) % 8 == 0
    dyT = ops.transpose_bf16(dy_b, pad_to=128, colsum=grads[id(bias)].view(-1) if fused_bias else None)   # [D, Mp] (+ db)
    xT = ops.transpose_bf16(x_bf16, pad_to=128)         # [K, Mp]
    Mp = dyT.shape[1]
    split = 1 if ordered else max(1, min(32, Mp // 2048))
    gw = grads[id(weight)]
    if Mp >= 4096 and ops.gemm_nt_splitk(dyT, xT, gw, accumulate=True):
        pass  # long contraction (MLM decoder over all tokens): 256x256 split-K workspace path
    elif split > 1:
        ops.gemm_nt(dyT, xT, out_f32=gw, split_k=split)      # atomically accumulates into the zeroed bucket
    else:
        ops.gemm_nt(dyT, xT, out_f32=gw, residual=gw)        # accumulate in place
    if not fused_bias:
        ops.colsum_bf16(dy_b, grads[id(bias)], **_ordered(ordered))
    w_t = ops.cast_transpose_bf16(_f32c(weight))   # [K, D]
    if D % 64 != 0:
        # a head width that is no multiple of the GEMM's K tile (timm's 1000-class head under SimCLR): zero-pad the contraction
        Dp = (D + 63) // 64 * 64
        dy_p, w_p = dy_b.new_zeros((M, Dp)), w_t.new_zeros((K, Dp))
        dy_p[:, :D].copy_(dy_b)
        w_p[:, :D].copy_(w_t)
        dy_b, w_t = dy_p, w_p
    if out_bf16:
        dx = torch.empty((M, K), dtype=BF16, device=dy_b.device)
        ops.gemm_nt(dy_b, w_t, out_bf16=dx)
    else:
        dx = torch.empty((M, K), dtype=F32, device=dy_b.device)
        ops.gemm_nt(dy_b, w_t, out_f32=dx)
    return dx
