"""Masked-k-mer pre-training of the BarcodeBERT DNA tower on the MI355X HIP engine: the link between a collection of barcodes and the
checkpoint `load_pre_trained_bioscan_bert` reads (`bioscan_bert_checkpoint`), as `clibd_amd.simclr` is for the image tower.

The objective is HF `BertForMaskedLM(input_ids, attention_mask, labels).loss` — what the reference instantiates (model/dna_encoder.py:35-37)
— with labels = -100 outside the masked positions: mean cross-entropy over the masked k-mers.  Two call forms: the project's own
`model(masked_ids, rows, targets, n_valid)`, and HF's `model(input_ids=, attention_mask=, labels=, label_capacity=)` (below).  The tower is `clibd_amd.towers.BertTower` under full
fine-tuning with head="hidden" (post-LN stack, embedding gradients, train-mode dropout, deterministic mode: all the DNA tower's); the
vocabulary head runs on the MASKED rows only: gather -> transform dense + GELU -> LayerNorm -> decoder GEMM to bf16 logits -> the fused
cross-entropy of csrc/mlm.hip, which leaves the gradient in the logits' place; the backward is the mirror and ends in a scatter into the
[B*S, H] gradient of the top hidden state.  bf16 GEMM operands, fp32 accumulation, statistics, loss and master weights.

The sampler (csrc/mlm.hip, `mask_tokens`): per sequence n_mask = max(1, int(mask_ratio * (S - 1))) positions; position 0 — the 0
`get_sequence_pipeline` prepends — is never chosen; position s >= 1 of sequence b gets the key (id == unk_id, lowbias32((b*S + s) ^
seed), s) and the n_mask smallest keys are chosen, so padding k-mers are taken only when real ones run out; a chosen id becomes mask_id,
its target the original id, or -100 where that was unk_id.  BarcodeBERT's own training code is not part of the reference, so this rule is
this project's and is pinned by the restatement in tests/mlm_reference.py.

HF-style labels.  `labels [B, S]` int64 with -100 = ignore and any number of labelled positions per sequence (position 0 and padded
positions included) are compacted on the device (csrc/mlm_labels.hip) into the ascending `rows` / `targets` the head runs on.  The
number of labelled rows is data, the head's GEMMs need a row count on the host, and nothing synchronises: the head runs at a capacity
R_cap, a multiple of 64 in 64 .. B S rounded up (`label_capacity`; None = B S rounded up, always enough).  The tail is padding: row
index -1 (gathered as zeros, never scattered), target -100 (zero loss, zero logit gradient).  More labelled positions than R_cap set the
sticky device word `model.label_overflow` and leave the first R_cap rows: a caller that passes a capacity must check that word
(`pretrain_epoch` does, in its one host fetch, and raises); nothing is truncated silently.  The loss divides by the number of labelled
positions, as HF's mean does.

The attention mask.  `attention_mask [B, S]`, nonzero = a live key, becomes the tower's int32 key mask and reaches the 64-wide masked
attention kernels in the forward and the backward, with and without dropout.  HF's semantics: a masked key gets probability 0; the
query rows of padded positions are still computed and matter only if labelled.  Every sequence must have at least position 0 live; an
all-zero row gives what the masked attention kernels define for it, which is not HF's result.  Towers with 128- or 192-wide heads raise
NotSupportedYet when a mask is passed (their kernels take full sequences only) and take labels and both samplers without one.

The 80/10/10 sampler (csrc/mlm_labels.hip, `mask_tokens_bert`): with i = b S + s, T(p) = floor(p 2^32 + 0.5) as a 64-bit integer and
u0 = lowbias32(i ^ seed), u1 = lowbias32(u0 + 0x9E3779B9), u2 = lowbias32(u0 + 2 * 0x9E3779B9) (mod 2^32): a position is eligible iff
s >= 1, its mask entry is nonzero and its id is no special id; it is chosen iff eligible and u0 < T(mlm_probability); a chosen id
becomes mask_id if u1 < T(replace[0]), else len(special_ids) + ((u2 (V - len(special_ids))) >> 32) — a uniform non-special id — if
u1 < T(replace[0]) + T(replace[1]), else stays; labels = the original id where chosen, -100 elsewhere.  A pure function of (seed, i):
no launch shape enters.  replace = (1, 0, 0) is plain masking.  Pinned by the numpy restatement in tests/mlm_labels_reference.py.

One stated divergence from a default-configured HF model: BertConfig's default pad_token_id = 0 is this vocabulary's <MASK>, which makes
row 0 of HF's word table an nn.Embedding padding row whose lookup gradient torch drops.  The embedding backward here has no padding row
(it never had one): the mask token's embedding trains through the lookup like every other row, as an HF model built with
pad_token_id=None does (the golden's models are built so).

Out of scope (each raises or simply does not exist here):
  - whole-word or span masking (the fixed-count sampler always writes mask_id; 80/10/10 replacement is `mask_tokens_bert`'s);
  - HF-style `labels [B, S]` beyond 2^24 positions, and an attention mask that is not [B, S] (no per-query or per-head masks);
  - the remote-code tokenizer of the newer BarcodeBERT checkpoints (strings go through the k-mer kernel, `eval.tokenize_barcodes`);
  - data-parallel pre-training over RCCL on more than one GPU is unmeasured (data-parallel pre-training itself: below and §3.18);
  - fp8 modes for this step;
  - S > 256 (S > 192 with 192-wide heads), and an attention mask with wide heads: full sequences only, as the towers.
The upstream gradient of the loss is taken as a device scalar; the loss's own gradient is written by the forward's cross-entropy kernel.

Large batches: gradient accumulation and data-parallel.  `pretrain_step` / `pretrain_epoch(..., accumulation_steps=k,
world_size=W, rank=r)` make k micro-batches on each of W ranks ONE update, the update of the batch k W times the size, exactly:
  - sum mode inside a window.  The cross-entropy gets a device word holding 1 as n_valid, so a micro-batch's loss is the SUM of its row
    losses and its gradient the sum's; the real count, that loss sum and the hits are added on the device into three spare slots of the
    optimizer's bucket (`aux[AUX_COUNT]`, `aux[AUX_LOSS]`, `aux[AUX_HITS]`).  Counts travel as fp32: exact up to 2^24 labelled positions
    per window, which is not checked;
  - the window's divisor is the GLOBAL labelled count (`optimizer.divisor_slot = AUX_COUNT`, `ops.grad_norm_div`): a token-weighted mean over
    all micro-batches and ranks — what one big batch computes, and what recent HF versions compute through `num_items_in_batch`.  It
    differs from DDP's mean of per-rank means (and from the classic mean of micro-batch means) whenever the counts differ;
  - data parallel: once per window, after the closing backward, ONE `dist.all_reduce(optimizer.flat_comm)` (SUM) carries gradients, count,
    loss sum and hits; grad_scale = 1; no other collective per step.  `pretrain_epoch` broadcasts rank 0's `flat_p` at its start and
    invalidates the tower's weight images, as `train.Trainer` does.  Sharding the data is the caller's job (DistributedSampler, as in the
    reference).  Over RCCL on more than one GPU this path is unmeasured;
  - mask seeds and dropout bases differ between ranks and micro-steps: both come from `micro_seed(seed, rank, micro-step)` (seed=None: a
    value drawn from the CPU generator, the same on equally seeded ranks); the tower draws its dropout base from a forked CPU generator
    seeded with it;
  - `scheduler.step()` runs once per applied window, `optimizer.flush()` at the epoch's end; the returned loss is sum of row losses / sum
    of counts over the whole epoch and all ranks, "steps" counts updates.
With k = 1 and W = 1 every launch, the returned dict and every bit of the parameters are what they were.  `evaluate` scores a held-out set.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import ops
from .engine import BF16, F32, GradBucket, NotSupportedYet, _f32c, _ordered, linear_wgrad, ln_param_grads
from .towers import BertTower

CONFIG_KEYS = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "max_position_embeddings",
               "layer_norm_eps", "hidden_dropout_prob", "attention_probs_dropout_prob")


def n_mask_for(S: int, mask_ratio: float) -> int:
    if not 0.0 < mask_ratio <= 1.0:
        raise ValueError("mask_ratio must be in (0, 1]")
    return max(1, int(mask_ratio * (S - 1)))


def mask_tokens(ids: torch.Tensor, mask_ratio: float = 0.5, seed: Optional[int] = None, mask_id: int = 0, unk_id: int = 2):
    """ids int64 [B, S] on the device -> (masked_ids [B, S], rows int32 [B * n_mask], targets int64 [B * n_mask], n_valid int32 [1]), all
    on the device (the module docstring has the rule).  seed=None draws it from the CPU generator, as the towers draw their dropout
    base: reproducible under torch.manual_seed, and no device synchronisation."""
    if ids.dim() != 2:
        raise ValueError("mask_tokens: ids must be [B, S]")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    return ops.mlm_mask(ids.to(torch.int64).contiguous(), seed, n_mask_for(ids.shape[1], mask_ratio), mask_id, unk_id)


def mask_tokens_bert(ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, mlm_probability: float = 0.15, seed: Optional[int] = None,
                     mask_id: int = 0, special_ids=(0, 1, 2), replace=(0.8, 0.1, 0.1), vocab_size=None):
    """BERT's sampler with 80/10/10 replacement (the module docstring has the rule): ids int64 [B, S] on the device -> (masked_ids,
    labels), both int64 [B, S] on the device, labels = -100 off the chosen positions.  Never chosen: position 0, positions with a zero
    attention_mask, ids in special_ids.  vocab_size: the vocabulary size V, or the model to take it from; it may be left out only when
    replace[1] == 0 (no random replacement is ever drawn).  seed=None draws it from the CPU generator, as `mask_tokens` does."""
    if ids.dim() != 2:
        raise ValueError("mask_tokens_bert: ids must be [B, S]")
    if vocab_size is None:
        if replace[1] != 0:
            raise ValueError("mask_tokens_bert: random replacement needs vocab_size (an int, or the model)")
        V = len(special_ids) + 1
    elif isinstance(vocab_size, int):
        V = vocab_size
    else:
        V = vocab_size.bert.embeddings.word_embeddings.weight.shape[0]
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    return ops.mlm_mask_bert(ids.to(torch.int64).contiguous(), attention_mask, V, seed, mlm_probability, mask_id, special_ids, replace)


def barcode_attention_mask(ids: torch.Tensor, unk_id: int = 2) -> torch.Tensor:
    """The attention mask of N-padded barcodes, int32 [B, S] on ids' device: a barcode shorter than the batch's window is padded with N,
    whose k-mers are <UNK>, so the TRAILING run of <UNK> ids of a sequence is its padding and everything before it is live — an <UNK>
    inside the barcode (an ambiguous base) stays a live key, as in the reference's tokenizer, which pads after tokenizing.  Position 0
    is always live."""
    live = (ids != unk_id).flip(1).to(torch.int32).cummax(dim=1).values.flip(1)
    live[:, 0] = 1
    return live.contiguous()


class _MLMFn(torch.autograd.Function):
    """forward(owner, masked_ids, rows, targets, n_valid, key_mask, *trainable parameters) -> (loss, correct)"""

    @staticmethod
    def forward(ctx, owner, masked_ids, rows, targets, n_valid, key_mask, *params):
        loss, correct, state = owner._forward(masked_ids, rows, targets, n_valid, True, key_mask)
        ctx.owner, ctx.state, ctx.nparams = owner, state, len(params)
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, dloss, _dcorrect):
        owner, state = ctx.owner, ctx.state
        if state is None:
            raise RuntimeError("backward twice through one pre-training forward")
        ctx.state = None
        params = owner.trainable_params()
        assert len(params) == ctx.nparams
        sink = owner.grad_sink
        if sink is not None and all(id(p) in sink for p in params):
            owner._backward(dloss, state, sink)   # the optimizer's flat bucket (clibd_amd.optim.FusedAdamW): accumulate straight into it
            return (None,) * (6 + len(params))
        bucket = GradBucket(params)
        owner._backward(dloss, state, bucket.views)
        return (None, None, None, None, None, None, *bucket.ordered())


class BarcodeBERTForPreTraining(nn.Module):
    """`model`: a BertForMaskedLM — the parameter container of clibd_amd.model or transformers' class; only parameters are read.  Every
    parameter is trainable (no LoRA).  `state_dict()` has exactly the HF keys (`bert. ...`, `cls.predictions. ...`).
    tie_word_embeddings: None reads `model.config.tie_word_embeddings` (absent: True, HF's default).  Tied: `cls.predictions.decoder.weight`
    IS the word-embedding Parameter and `decoder.bias` IS `cls.predictions.bias`, as in HF; both names stay in the state dict.  Untied:
    four separate parameters (`cls.predictions.bias` then takes no part, as in HF)."""

    def __init__(self, model, tie_word_embeddings: Optional[bool] = None):
        super().__init__()
        self.bert, self.cls, self.config = model.bert, model.cls, getattr(model, "config", None)
        if tie_word_embeddings is None:
            tie_word_embeddings = bool(getattr(self.config, "tie_word_embeddings", True))
        self.tie_word_embeddings = bool(tie_word_embeddings)
        pred = self.cls.predictions
        word = self.bert.embeddings.word_embeddings.weight
        if tuple(pred.decoder.weight.shape) != tuple(word.shape):
            raise ValueError("BarcodeBERTForPreTraining: the decoder must span the vocabulary (a replaced decoder is a fine-tuned tower)")
        if self.tie_word_embeddings:
            pred.decoder.weight = word
            pred.decoder.bias = pred.bias
        elif pred.decoder.weight is word or pred.decoder.bias is pred.bias:
            raise ValueError("BarcodeBERTForPreTraining: the model is tied; untie it before asking for tie_word_embeddings=False")
        if any(hasattr(l.attention.self.query, "w_a") for l in self.bert.encoder.layer):
            raise NotSupportedYet("BarcodeBERTForPreTraining: LoRA adapters (pre-training is a full fine-tune)")
        V, H = word.shape
        if V > 8192 or H % 64:
            raise NotSupportedYet(f"BarcodeBERTForPreTraining: vocabulary {V} > 8192 (k <= 6) or a hidden size {H} that is no multiple of 64")
        for p in self.parameters():
            p.requires_grad_(True)
        self.grad_sink = None   # {id(param): fp32 accumulation tensor}: see attach()
        self._tower = None
        self._label_overflow = None

    @property
    def label_overflow(self) -> torch.Tensor:
        """int32 [1] on the parameters' device, sticky: bit 0 is set once an HF-style call met more labelled positions than its capacity.
        Reading it is a host synchronisation; `.zero_()` re-arms it."""
        dev = self.bert.embeddings.word_embeddings.weight.device
        if self._label_overflow is None or self._label_overflow.device != dev:
            self._label_overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
        return self._label_overflow

    def tower(self) -> BertTower:
        if self._tower is None:
            self._tower = BertTower(self.bert, "hidden", {})
        return self._tower

    def set_deterministic(self, enabled: bool = True):
        """fixed-order reductions in the whole backward (clibd_amd.engine.default_deterministic): the same weights, batch, mask and dropout
        seeds give the same loss, gradients and update bit for bit.  Under tying the decoder's weight gradient goes into the shared
        buffer first, the embedding-lookup gradient second, in every mode."""
        self.tower().deterministic = bool(enabled)
        return self

    def attach(self, optimizer):
        """wire a clibd_amd.optim.FusedAdamW built over `self.parameters()`: the backward accumulates into its flat gradient bucket"""
        if not hasattr(optimizer, "flat_g"):
            raise NotSupportedYet("BarcodeBERTForPreTraining.attach: needs clibd_amd.optim.FusedAdamW (the flat gradient bucket)")
        self.grad_sink = {id(p): p.grad for p in optimizer.bucket_params()}
        return self

    def _head(self):
        pred = self.cls.predictions
        return pred.transform.dense, pred.transform.LayerNorm, pred.decoder

    def trainable_params(self):
        """the tower's parameters, then the head's; a tied parameter once"""
        td, tln, dec = self._head()
        ps, seen = [], set()
        for p in self.tower().trainable_params() + [td.weight, td.bias, tln.weight, tln.bias, dec.weight, dec.bias]:
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                ps.append(p)
        return ps

    def forward(self, masked_ids=None, rows=None, targets=None, n_valid=None, *, input_ids=None, attention_mask=None, labels=None,
                label_capacity: Optional[int] = None):
        """(loss fp32 scalar, correct int32 [1]) on the device; under autograd `loss.backward()` produces every parameter gradient.
        Two forms:
          model(masked_ids, rows, targets, n_valid)          the sampler's rows (`mask_tokens`);
          model(input_ids=, attention_mask=, labels=, label_capacity=)     HF's: labels int64 [B, S], -100 = ignore, any number of labelled
              positions per sequence; the loss is the mean cross-entropy over them.  label_capacity: the row capacity of the head, a
              multiple of 64 in 64 .. B S rounded up; None = B S rounded up, which always suffices.  A caller that passes a smaller one
              must check `model.label_overflow` (a device tensor, sticky): when more positions are labelled the first `label_capacity`
              of them are used and that word is set; no host synchronisation happens here.
        attention_mask ([B, S], nonzero = a live key; either form): HF's semantics, every sequence with at least position 0 live; 64-wide
        heads only (wider towers raise NotSupportedYet)."""
        if labels is not None or input_ids is not None:
            if labels is None or input_ids is None or any(a is not None for a in (masked_ids, rows, targets, n_valid)):
                raise TypeError("BarcodeBERTForPreTraining: pass either (masked_ids, rows, targets, n_valid) or input_ids= and labels=")
            if input_ids.dim() != 2 or tuple(labels.shape) != tuple(input_ids.shape):
                raise ValueError("BarcodeBERTForPreTraining: input_ids and labels must both be [B, S]")
            V = self.bert.embeddings.word_embeddings.weight.shape[0]
            masked_ids = input_ids
            rows, targets, n_valid = ops.mlm_compact_labels(labels.to(torch.int64).contiguous(), V, label_capacity, overflow=self.label_overflow)
        elif label_capacity is not None:
            raise TypeError("BarcodeBERTForPreTraining: label_capacity belongs to the labels= form")
        key_mask = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != tuple(masked_ids.shape):
                raise ValueError("BarcodeBERTForPreTraining: attention_mask must be [B, S]")
            key_mask = (attention_mask != 0).to(torch.int32).contiguous()
        params = self.trainable_params()
        if torch.is_grad_enabled() and params:
            return _MLMFn.apply(self, masked_ids, rows, targets, n_valid, key_mask, *params)
        with torch.no_grad():
            loss, correct, _ = self._forward(masked_ids, rows, targets, n_valid, False, key_mask)
        return loss, correct

    def _forward(self, masked_ids, rows, targets, n_valid, save, key_mask=None):
        tw = self.tower()
        tw.training = self.training
        if tw.stack.fp8 is not None:
            raise NotSupportedYet("BarcodeBERTForPreTraining: the fp8 forward")
        x_top, state = tw._forward((masked_ids, None, key_mask), save)   # [M, H] bf16
        loss, correct, head = self._head_forward(x_top, rows, targets, n_valid)
        if save:
            state.update(mlm=head)
        return loss, correct, state

    def _head_forward(self, x_top, rows, targets, n_valid):
        """the vocabulary head on the rows `rows` of x_top bf16 [M, H]: (loss, correct, what the backward needs)"""
        td, tln, dec = self._head()
        M, H = x_top.shape
        dev = x_top.device
        rows = rows.to(torch.int32).contiguous()
        R = rows.numel()
        xg = ops.rows_gather(x_top, rows)
        wt = ops.cast_bf16(_f32c(td.weight))
        hpre = torch.empty((R, H), dtype=BF16, device=dev)
        g = torch.empty((R, H), dtype=F32, device=dev)
        ops.gemm_nt(xg, wt, bias=_f32c(td.bias), act=ops.ACT_GELU, out_pre=hpre, out_f32=g)
        hln = torch.empty((R, H), dtype=BF16, device=dev)
        st = torch.empty((R, 2), dtype=F32, device=dev)
        ops.layernorm_fwd(g, _f32c(tln.weight), _f32c(tln.bias), float(tln.eps), y_bf16=hln, stats=st)
        # the decoder over a vocabulary that is no multiple of the GEMM's tiles (4^k + 3): zero rows pad the weight image to a multiple of
        # 64 — the N granule of the forward and the K granule of the dgrad — and the cross-entropy never reads the padding columns
        V = dec.weight.shape[0]
        Vp = (V + 63) // 64 * 64
        wp, bp = torch.zeros((Vp, H), dtype=BF16, device=dev), torch.zeros((Vp,), dtype=F32, device=dev)
        wp[:V].copy_(ops.cast_bf16(_f32c(dec.weight)))
        bp[:V].copy_(_f32c(dec.bias))
        logits = torch.empty((R, Vp), dtype=BF16, device=dev)
        ops.gemm_nt(hln, wp, bias=bp, out_bf16=logits)
        loss, correct, _ = ops.mlm_ce_(logits, V, targets.to(torch.int64).contiguous(), n_valid)   # logits now holds d loss / d logits
        return loss.reshape(()), correct, dict(rows=rows, xg=xg, hpre=hpre, g=g, st=st, hln=hln, dlogits=logits, wp=wp, M=M, V=V)

    def _backward(self, dloss, state, grads):
        dx = self._head_backward(dloss, state.pop("mlm"), grads)
        self.tower()._backward(dx, state, grads)

    def _head_backward(self, dloss, s, grads):
        """the head's parameter gradients into `grads` (accumulating); returns the gradient of the top hidden state, bf16 [M, H]"""
        td, tln, dec = self._head()
        det = self.tower().deterministic
        dl, hln, V, M = s["dlogits"], s["hln"], s["V"], s["M"]
        R, H = hln.shape
        dev = dl.device
        dl.mul_(dloss.detach().reshape(()).to(BF16))   # the upstream gradient (loss.backward(): exactly 1)
        # decoder: dW [V, H] += dlogits^T hln (under tying into the word table's buffer, ahead of the lookup gradient), db += column sums
        csum = torch.zeros((dl.shape[1],), dtype=F32, device=dev)
        dyT = ops.transpose_bf16(dl, pad_to=128, colsum=csum if id(dec.bias) in grads else None)   # [Vp, Rp] (+ fixed-order column sums)
        if id(dec.bias) in grads:
            grads[id(dec.bias)].view(-1).add_(csum[:V])
        if id(dec.weight) in grads:
            xT = ops.transpose_bf16(hln, pad_to=128)   # [H, Rp]
            Rp = dyT.shape[1]
            gw = grads[id(dec.weight)].view(V, H)
            split = 1 if det else max(1, min(32, Rp // 2048))
            if Rp >= 4096 and ops.gemm_nt_splitk(dyT[:V], xT, gw, accumulate=True):
                pass   # long contraction: the 256x256 split-K workspace path, partials summed in a fixed order
            elif split > 1:
                ops.gemm_nt(dyT[:V], xT, out_f32=gw, split_k=split)
            else:
                ops.gemm_nt(dyT[:V], xT, out_f32=gw, residual=gw)
        dhln = torch.empty((R, H), dtype=BF16, device=dev)
        ops.gemm_nt(dl, ops.transpose_bf16(s["wp"], pad_to=64), out_bf16=dhln)   # [R, Vp] x ([H, Vp])^T: the padding contracts zeros
        dg = torch.empty((R, H), dtype=BF16, device=dev)
        ops.layernorm_bwd(dhln, s["g"], s["st"], _f32c(tln.weight), dx_bf16=dg, **ln_param_grads(grads, tln.weight, tln.bias, det))
        dhpre = ops.gelu_bwd(dg, s["hpre"])
        linear_wgrad(dhpre, s["xg"], [td.weight], [td.bias], grads, **_ordered(det))
        dxg = torch.empty((R, H), dtype=BF16, device=dev)
        ops.gemm_nt(dhpre, ops.cast_transpose_bf16(_f32c(td.weight)), out_bf16=dxg)
        return ops.rows_scatter(dxg, s["rows"], M)   # zeros in the rows that were not masked


def _ids_of(batch, device, k: int) -> torch.Tensor:
    if isinstance(batch, torch.Tensor):
        return batch.to(device=device, dtype=torch.int64)
    if isinstance(batch, (list, tuple)) and batch and all(isinstance(s, str) for s in batch):
        from .eval import tokenize_barcodes

        return tokenize_barcodes(list(batch), device, k=k)
    raise TypeError("pre-training batches are int64 [b, S] token ids, (ids, attention_mask) pairs or lists of barcode strings")


def _kmer_k(model) -> int:
    V = model.bert.embeddings.word_embeddings.weight.shape[0]
    for k in range(1, 7):
        if 4 ** k + 3 == V:
            return k
    raise NotSupportedYet(f"a vocabulary of {V} entries is not <MASK>, <CLS>, <UNK> + 4^k k-mers: pass token ids")


AUX_COUNT, AUX_LOSS, AUX_HITS = 1, 2, 3   # slots of FusedAdamW.aux (slot 0 is train.Trainer's loss): labelled count, loss sum, hits, fp32
_ones = {}


def _one(dev) -> torch.Tensor:
    """a device int32 [1] holding 1: as the cross-entropy's n_valid it turns the mean into the sum (never written)"""
    dev = torch.device(dev)
    if dev not in _ones:
        _ones[dev] = torch.ones((1,), dtype=torch.int32, device=dev)
    return _ones[dev]


def micro_seed(seed: int, rank: int, micro_step: int) -> int:
    """the 31-bit seed of micro-step `micro_step` on rank `rank`: lowbias32 over the three values chained, so that neither two ranks
    nor two micro-steps share a mask or a dropout pattern.  A pure function (tests restate the masks from it)."""
    x = int(seed) & 0xFFFFFFFF
    for v in (int(rank) + 1, int(micro_step) + 1):
        x = (x ^ (v * 0x9E3779B1)) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
    return x & 0x7FFFFFFF


def _batch_inputs(model, batch, attention_mask, labels, who: str):
    """(ids on the device, attention_mask on the device or None, labels or None, whether the batch was barcode strings).  A dict is an
    HF collator's batch: "input_ids", and optionally "attention_mask" and "labels"."""
    dev = next(model.parameters()).device
    strings = False
    if isinstance(batch, dict):
        if (attention_mask is not None and batch.get("attention_mask") is not None) or (labels is not None and batch.get("labels") is not None):
            raise TypeError(f"{who}: an attention mask or labels in the batch and another as an argument")
        attention_mask = batch.get("attention_mask") if attention_mask is None else attention_mask
        labels = batch.get("labels") if labels is None else labels
        batch = batch["input_ids"]
    elif isinstance(batch, (list, tuple)) and len(batch) == 2 and all(isinstance(t, torch.Tensor) for t in batch):
        if attention_mask is not None:
            raise TypeError(f"{who}: an attention mask in the batch and another as an argument")
        batch, attention_mask = batch
    elif not isinstance(batch, torch.Tensor):
        strings = True
    ids = _ids_of(batch, dev, _kmer_k(model) if strings else 0)
    if attention_mask is not None:
        attention_mask = attention_mask.to(dev)
    return ids, attention_mask, labels, strings


def _sample(model, ids, attention_mask, strings, sampler, mask_ratio, mlm_probability, label_capacity, seed, labels, who: str):
    """(masked ids, rows, targets, n_valid, attention_mask) of one batch: the fixed-count sampler, BERT's, or the caller's own `labels`"""
    V = model.bert.embeddings.word_embeddings.weight.shape[0]
    if labels is not None:
        if tuple(labels.shape) != tuple(ids.shape):
            raise ValueError(f"{who}: labels must be [b, S] like the ids")
        rows, targets, n_valid = ops.mlm_compact_labels(labels.to(device=ids.device, dtype=torch.int64).contiguous(), V, label_capacity,
                                                        overflow=model.label_overflow)
        return ids, rows, targets, n_valid, attention_mask
    if sampler == "fixed":
        if label_capacity is not None:
            raise TypeError(f'{who}: label_capacity belongs to sampler="bert"')
        masked, rows, targets, n_valid = mask_tokens(ids, mask_ratio, seed)
        return masked, rows, targets, n_valid, attention_mask
    if strings and attention_mask is None:
        attention_mask = barcode_attention_mask(ids)
    masked, labels = mask_tokens_bert(ids, attention_mask, mlm_probability, seed, vocab_size=model)
    if label_capacity is None:
        label_capacity = ops.mlm_label_capacity(ids.numel(), mlm_probability)
    rows, targets, n_valid = ops.mlm_compact_labels(labels, V, label_capacity, overflow=model.label_overflow)   # keeps the count for the caller
    return masked, rows, targets, n_valid, attention_mask


def _window_of(optimizer, accumulation_steps, world_size, who: str):
    """(k, exact): k from the argument or the optimizer; exact = the sum-mode window (k > 1 or W > 1), which needs the flat bucket"""
    have = getattr(optimizer, "accumulation_steps", 1)
    k = have if accumulation_steps is None else int(accumulation_steps)
    if k < 1 or int(world_size) < 1:
        raise ValueError(f"{who}: accumulation_steps and world_size must be >= 1")
    exact = k > 1 or int(world_size) > 1
    if exact and not hasattr(optimizer, "divisor_slot"):
        raise NotSupportedYet(f"{who}: accumulation_steps > 1 or world_size > 1 needs clibd_amd.optim.FusedAdamW / FusedAdam (the flat "
                              "gradient bucket is the accumulator and the all-reduce message)")
    if k != have:
        if getattr(optimizer, "window_open", False):
            raise ValueError(f"{who}: accumulation_steps={k} in the middle of the optimizer's window of {have}")
        optimizer.accumulation_steps = k
    return k, exact


def pretrain_step(model: BarcodeBERTForPreTraining, batch, optimizer, mask_ratio: float = 0.5, seed: Optional[int] = None, sampler: str = "fixed",
                  mlm_probability: float = 0.15, attention_mask: Optional[torch.Tensor] = None, label_capacity: Optional[int] = None,
                  accumulation_steps: Optional[int] = None, world_size: int = 1, rank: int = 0, labels: Optional[torch.Tensor] = None):
    """mask -> forward -> backward -> optimizer step on one batch; returns the device tensors (loss, correct, n_valid).  No host
    synchronisation.
    batch: token ids int64 [b, S], a pair (ids, attention_mask), a list of barcode strings, or an HF collator's dict ("input_ids", and
        optionally "attention_mask" and "labels": with labels the ids are used as they are, see labels= below).
    sampler="fixed" (the default): `mask_tokens` at `mask_ratio`, exactly n_mask rows per sequence; an attention mask, if one is given,
        reaches the encoder; barcode strings get none (as before).
    sampler="bert": `mask_tokens_bert` at `mlm_probability` with 80/10/10 replacement and HF-style labels.  Barcode strings get the
        mask of `barcode_attention_mask` (the trailing <UNK> run of a sequence is padding).  label_capacity=None: ceil(b S min(1, p +
        6 sqrt(p (1 - p) / (b S)))) rounded up to 64 — six binomial standard deviations over the mean.  Overflow sets
        `model.label_overflow`; `pretrain_epoch` raises on it.
    labels= (HF-style int64 [b, S], -100 = ignore): the caller's own collator; the ids are used as they are and no sampler runs
        (label_capacity=None: b S rounded up).
    accumulation_steps=k (None: the optimizer's), world_size=W, rank=r: with k > 1 or W > 1 this call is ONE MICRO-STEP of a window of k
        (the module docstring has the rule).  The loss runs in sum mode: the returned loss is the micro-batch's SUM of row losses, and
        `optimizer.aux[AUX_COUNT], [AUX_LOSS], [AUX_HITS]` hold the window's totals (all ranks', once the window has closed) until the next
        window opens.  The closing micro-step issues the one all-reduce (W > 1) and the update; `optimizer.window_closes` tells which.
        The process group must exist; sharding the data and broadcasting the parameters (`pretrain_epoch` does the latter) are the caller's."""
    if sampler not in ("fixed", "bert"):
        raise ValueError('pretrain_step: sampler is "fixed" or "bert"')
    k, exact = _window_of(optimizer, accumulation_steps, world_size, "pretrain_step")
    ids, attention_mask, labels, strings = _batch_inputs(model, batch, attention_mask, labels, "pretrain_step")
    optimizer.zero_grad()
    if not exact:
        masked, rows, targets, n_valid, attention_mask = _sample(model, ids, attention_mask, strings, sampler, mask_ratio, mlm_probability,
                                                                 label_capacity, seed, labels, "pretrain_step")
        loss, correct = model(masked, rows, targets, n_valid, attention_mask=attention_mask)
        loss.backward()
        optimizer.step()
        return loss.detach(), correct, n_valid
    optimizer.divisor_slot, optimizer.grad_scale = AUX_COUNT, 1.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())   # the CPU generator: the same value on equally seeded ranks
    micro = optimizer.step_count * k + optimizer.micro_steps
    masked, rows, targets, n_valid, attention_mask = _sample(model, ids, attention_mask, strings, sampler, mask_ratio, mlm_probability,
                                                             label_capacity, micro_seed(seed, rank, micro), labels, "pretrain_step")
    with torch.random.fork_rng(devices=[]):   # the tower draws its dropout base from the CPU generator: give it this rank's and micro-step's
        torch.manual_seed(micro_seed(seed ^ 0x5DEECE66, rank, micro))
        loss, correct = model(masked, rows, targets, _one(ids.device), attention_mask=attention_mask)   # n_valid = 1: the sum of the row losses
    optimizer.aux[AUX_COUNT : AUX_HITS + 1].add_(torch.cat([n_valid.to(F32), loss.detach().reshape(1), correct.to(F32)]))
    loss.backward()
    if optimizer.window_closes and world_size > 1:
        torch.distributed.all_reduce(optimizer.flat_comm)   # SUM: gradients, count, loss sum and hits in one message, once per window
    optimizer.step()
    return loss.detach(), correct, n_valid


def _broadcast_parameters(model, optimizer):
    """rank 0's parameters to every rank (train.Trainer.__init__'s rule): the trainable values are one message, the rest follow tensor
    by tensor; `.data` writes do not bump Parameter._version, so the tower's bf16 weight images are dropped explicitly"""
    import torch.distributed as dist

    dist.broadcast(optimizer.flat_p, src=0)
    own = {id(p) for p in optimizer.bucket_params()}
    with torch.no_grad():
        for t in list(model.parameters()) + list(model.buffers()):
            if id(t) not in own:
                dist.broadcast(t.data, src=0)
    tw = model.tower()
    if hasattr(tw, "invalidate_weight_images"):
        tw.invalidate_weight_images()


def pretrain_epoch(model: BarcodeBERTForPreTraining, loader, optimizer, scheduler=None, mask_ratio: float = 0.5, log_every: int = 0,
                   sampler: str = "fixed", mlm_probability: float = 0.15, label_capacity: Optional[int] = None,
                   accumulation_steps: Optional[int] = None, world_size: int = 1, rank: int = 0, seed: Optional[int] = None,
                   broadcast_parameters: bool = True):
    """One pass over `loader` (int64 [b, S] ids, (ids, attention_mask) pairs or lists of barcode strings) in train mode; `sampler`,
    `mlm_probability` and `label_capacity` as in `pretrain_step`.  `optimizer`: clibd_amd.optim.FusedAdamW over
    model.parameters(), wired to the backward here as simclr.py wires its own; `scheduler` (optional) is stepped per batch.  The loss and
    the masked-token hits accumulate on the device and are fetched once, at the end (log_every > 0 fetches the running mean every that many
    steps, a host synchronisation each); the same fetch reads `model.label_overflow` and raises RuntimeError if a step met more labelled
    positions than its capacity, and `optimizer.skipped_steps` (clibd_amd.optim, nonfinite="skip").  Returns {"loss": mean step loss,
    "accuracy": hits / valid targets, "steps": n, "skipped": steps this epoch dropped for a non-finite gradient norm (0 for an optimizer
    without the counter)}.  A skipped step still counts in "steps" and its loss still enters the mean, so a NaN loss shows there.

    accumulation_steps=k (None: the optimizer's), world_size=W, rank=r, seed (None: drawn per micro-step from the CPU generator): with
    k > 1 or W > 1 every batch of `loader` is a micro-batch (the module docstring has the rule): the scheduler is stepped once per applied
    window, a partial window at the loader's end is applied (`optimizer.flush()`, after its all-reduce; every rank must see the same
    number of batches), "loss" is the sum of row losses / the sum of labelled counts over the epoch and over all ranks, "accuracy" likewise,
    "steps" counts updates, and log_every counts updates too.  W > 1: rank 0's parameters are broadcast first
    (broadcast_parameters=False when the caller has done it)."""
    if hasattr(optimizer, "flat_g"):
        model.attach(optimizer)
    model.train()
    dev = next(model.parameters()).device
    k, exact = _window_of(optimizer, accumulation_steps, world_size, "pretrain_epoch")
    acc = torch.zeros((3,), dtype=torch.float64, device=dev)   # sum of step losses, hits, valid targets
    n = 0
    counter = getattr(optimizer, "skipped_steps", None)
    skipped0 = counter.clone() if counter is not None else torch.zeros((1,), dtype=torch.int32, device=dev)   # a device copy, no fetch
    if not exact:
        for batch in loader:
            loss, correct, n_valid = pretrain_step(model, batch, optimizer, mask_ratio, sampler=sampler, mlm_probability=mlm_probability,
                                                   label_capacity=label_capacity)
            acc += torch.stack([loss.double(), correct[0].double(), n_valid[0].double()])
            n += 1
            if scheduler is not None:
                scheduler.step()
            if log_every and n % log_every == 0:
                s = acc.tolist()
                print(f"step {n}\tloss {s[0] / n:.4f}\tmasked-token accuracy {s[1] / max(s[2], 1.0):.4f}")
    else:
        if world_size > 1 and broadcast_parameters:
            _broadcast_parameters(model, optimizer)
        if optimizer.window_open:
            raise ValueError("pretrain_epoch: the optimizer is in the middle of a window")

        def applied():   # the window's totals (all ranks') sit in aux until the next zero_grad
            nonlocal n
            acc.add_(torch.stack([optimizer.aux[AUX_LOSS].double(), optimizer.aux[AUX_HITS].double(), optimizer.aux[AUX_COUNT].double()]))
            n += 1
            if scheduler is not None:
                scheduler.step()
            if log_every and n % log_every == 0:
                s = acc.tolist()
                print(f"update {n}\tloss {s[0] / max(s[2], 1.0):.4f}\tmasked-token accuracy {s[1] / max(s[2], 1.0):.4f}")

        for batch in loader:
            pretrain_step(model, batch, optimizer, mask_ratio, seed=seed, sampler=sampler, mlm_probability=mlm_probability,
                          label_capacity=label_capacity, accumulation_steps=k, world_size=world_size, rank=rank)
            if not optimizer.window_open:
                applied()
        if optimizer.window_open:   # a partial window at the loader's end
            if world_size > 1:
                torch.distributed.all_reduce(optimizer.flat_comm)
            optimizer.flush()
            applied()
    skipped = (counter if counter is not None else skipped0) - skipped0
    s = torch.cat([acc, model.label_overflow.double(), skipped.double()]).tolist()   # the one host fetch of the epoch
    if s[3] != 0:
        model.label_overflow.zero_()
        raise RuntimeError("pretrain_epoch: a step labelled more positions than its label_capacity (model.label_overflow): rows were left "
                           "out of the loss; rerun with a larger capacity or label_capacity=None")
    if exact:
        return {"loss": s[0] / max(s[2], 1.0), "accuracy": s[1] / max(s[2], 1.0), "steps": n, "skipped": int(s[4])}
    return {"loss": s[0] / max(n, 1), "accuracy": s[1] / max(s[2], 1.0), "steps": n, "skipped": int(s[4])}


def evaluate(model: BarcodeBERTForPreTraining, loader, sampler: str = "fixed", seed: int = 0, world_size: int = 1, rank: int = 0,
             mask_ratio: float = 0.5, mlm_probability: float = 0.15, label_capacity: Optional[int] = None):
    """Score a held-out set: a no-grad, eval-mode pass over `loader` (the batch forms of `pretrain_step`); batch number i of rank r is
    masked by `sampler` with the seed `micro_seed(seed, r, i)`, so the same seed scores the same masks every time (a dict batch with
    "labels" is scored on those).  Returns the
    token-weighted {"loss": sum of row losses / labelled positions, "accuracy": hits / labelled positions, "perplexity": exp(loss),
    "tokens": labelled positions} over all batches (and all ranks: one all-reduce of the three sums under world_size > 1, each rank scoring
    its shard).  The sums accumulate on the device in fp64; one host fetch, which also checks `model.label_overflow` (RuntimeError).
    Parameters, optimizer state and the caller's train / eval mode are left as they were."""
    import math

    if sampler not in ("fixed", "bert"):
        raise ValueError('evaluate: sampler is "fixed" or "bert"')
    was_training = model.training
    model.eval()
    dev = next(model.parameters()).device
    acc = torch.zeros((3,), dtype=torch.float64, device=dev)   # sum of row losses, hits, labelled positions
    try:
        with torch.no_grad():
            for i, batch in enumerate(loader):
                ids, attention_mask, labels, strings = _batch_inputs(model, batch, None, None, "evaluate")
                masked, rows, targets, n_valid, attention_mask = _sample(model, ids, attention_mask, strings, sampler, mask_ratio, mlm_probability,
                                                                         label_capacity, micro_seed(seed, rank, i), labels, "evaluate")
                loss, correct = model(masked, rows, targets, _one(dev), attention_mask=attention_mask)   # n_valid = 1: the sum
                acc += torch.stack([loss.double(), correct[0].double(), n_valid[0].double()])
    finally:
        model.train(was_training)
    if world_size > 1:
        torch.distributed.all_reduce(acc)
    s = torch.cat([acc, model.label_overflow.double()]).tolist()   # the one host fetch
    if s[3] != 0:
        model.label_overflow.zero_()
        raise RuntimeError("evaluate: a batch labelled more positions than its label_capacity (model.label_overflow)")
    tokens = max(s[2], 1.0)
    loss = s[0] / tokens
    return {"loss": loss, "accuracy": s[1] / tokens, "perplexity": math.exp(loss) if loss < 700 else float("inf"), "tokens": int(s[2])}


def bert_config_of(model) -> dict:
    cfg = getattr(model, "config", None)
    if cfg is None:
        raise ValueError("save_pretrained: the model carries no config")
    out = {k: getattr(cfg, k) for k in CONFIG_KEYS}
    out["tie_word_embeddings"] = bool(getattr(model, "tie_word_embeddings", getattr(cfg, "tie_word_embeddings", True)))
    return out


def save_pretrained(model: BarcodeBERTForPreTraining, path) -> dict:
    """{"model": state dict with the HF keys (CPU tensors), "bert_config": {...}}: the file `load_pre_trained_bioscan_bert(path)` and
    `load_clip_model` (`bioscan_bert_checkpoint`) read unchanged.  Under tying the shared tensors are written under both names."""
    ckpt = {"model": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, "bert_config": bert_config_of(model)}
    torch.save(ckpt, path)
    return ckpt
