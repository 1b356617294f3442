"""Fused AdamW over one flat fp32 bucket (torch.optim.AdamW semantics; reference scripts/train_cl.py:221).

All trainable parameters (LoRA adapters, heads, logit_scale: 1.48 M values for I+D) are re-homed as views of ONE
contiguous buffer, and so are their gradients: the data-parallel all-reduce is a single RCCL call on the flat
gradient bucket and the update is a single kernel launch.  It is a real torch.optim.Optimizer, so
the reference's LR schedulers (OneCycleLR, CosineAnnealingLR, ... train_cl.py:222-246) drive every group's `lr`.

Beyond the plain update (include/clibd_hip_optim.h):
  - parameter groups: torch's list of group dicts with per-group `lr` and `weight_decay`, at most 8.  The bucket lays the groups out one
    after another, parameters in the given order inside each group; `bucket_params()` is that order.  `decay_parameter_groups(module,
    weight_decay)` makes HF Trainer's two groups (LayerNorm parameters and biases exempt from decay).
  - `max_grad_norm`: global L2-norm clipping, torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) of the averaged gradient, computed
    on the device in a fixed order (no float atomics: every run and every box give the same bits) and applied inside the update.
  - `nonfinite="propagate"` is torch's error_if_nonfinite=False: a NaN or inf norm flows into the update as it would after
    clip_grad_norm_.  `nonfinite="skip"` drops such a step on the device — parameters and both moments keep their bits — and counts it.
    `step_count` advances on the host for a skipped step too, because the host cannot know about it without a synchronisation, so the
    bias correction counts the skipped step: the one deviation from torch.amp.GradScaler, which does not advance the optimizer.
  - `grad_norm` (device fp32 [1], the pre-clip norm of the last step) and `skipped_steps` (device int32 [1]) are views of the 16-byte
    device record; the optimizer never fetches them.  They are written only by steps that clip or skip.
  - data-parallel: the norm is taken after the all-reduce, over the reduced bucket, with `grad_scale` folded in; every rank reads the same
    bucket and takes the same decision, so there is no new collective.
With no `max_grad_norm`, "propagate" and one group, `step()` is the single launch of `ops.adamw_step` / `ops.adam_l2_step` it always was.

Accumulation windows (include/clibd_hip_accum.h): `accumulation_steps=k`.  The driver goes on calling `zero_grad()` and
`step()` once per micro-batch: `zero_grad()` clears the bucket (and `aux`) only when a window opens, every backward adds into it, and
`step()` launches nothing until the k-th call of the window, which applies the window's gradient and advances `step_count` once.
`window_closes` says whether the next `step()` applies; `flush()` applies a partial window (an epoch's end).  The divisor:
  - by default the number of micro-steps taken, on the host, folded into `grad_scale`: the mean of the micro-batches' mean gradients, HF
    Trainer's classic semantics for micro-batches of equal size.  The launches are those of a k = 1 step on the same bucket with
    grad_scale / micro-steps;
  - `divisor_slot = i`: `aux[i]` on the device, read by `ops.grad_norm_div` — a count (fp32, exact to 2^24) that the driver summed there and
    that rode through the all-reduce with the gradients, e.g. the labelled positions of a masked-LM window (clibd_amd.mlm).  The update is
    then always the norm launch plus the grouped update, whose factor grad_scale * coef carries the division.
`max_grad_norm` and `nonfinite="skip"` act on the window's averaged gradient; a skipped window leaves p, m and v untouched.
`checkpoint.save_training_state` refuses in the middle of a window.  A driver that issues the bucket's all-reduce itself, per step
(`train.Trainer`, `simclr.SimCLR`), raises ValueError for accumulation_steps > 1 under world_size > 1: a bucket reduced twice is silently
wrong.  Accumulating a contrastive loss is not the loss of the large batch (the negatives of a micro-batch are its own), so the contrastive
`Trainer` does not use windows: its large-batch form is the chunked step, `Trainer(chunk_size=...)` / `SimCLR(chunk_size=...)` (clibd_amd.chunked,
DESIGN §3.19).  With accumulation_steps=1 and no divisor slot every launch is what it was.

Refused or not here: norm types other than 2, clipping by value, per-group betas or eps, amsgrad, maximize, more than 8 groups, LAMB and
LARS, gradient accumulation of a contrastive loss (gradient accumulation itself: above and §3.18; the contrastive large batch: the chunked step,
§3.19), a device-side step counter.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

MAX_GROUPS = 8  # CLIBD_OPTIM_MAX_GROUPS (include/clibd_hip_optim.h): the group table travels in the kernel arguments


class FusedAdamW(torch.optim.Optimizer):
    AUX_SLOTS = 64  # spare fp32 slots behind the gradients in the same allocation: scalars that ride along the gradient all-reduce

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm: Optional[float] = None,
                 nonfinite: str = "propagate", accumulation_steps: int = 1):
        name = type(self).__name__
        if isinstance(accumulation_steps, bool) or not isinstance(accumulation_steps, int) or accumulation_steps < 1:
            raise ValueError(f"{name}: accumulation_steps must be an integer >= 1")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"{name}: max_grad_norm must be positive (None: no clipping)")
        if nonfinite not in ("propagate", "skip"):
            raise ValueError(f'{name}: nonfinite is "propagate" or "skip"')
        params = list(params)
        if params and isinstance(params[0], dict):
            groups = []
            for grp in params:
                ps = [p for p in grp["params"] if p.requires_grad]
                if ps:   # a group whose parameters are all frozen owns no part of the bucket
                    groups.append({**grp, "params": ps})
            params = groups
        else:
            params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("FusedAdamW: no trainable parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"{name} supports at most {MAX_GROUPS} parameter groups")
        g0 = self.param_groups[0]
        if any(tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"] for g in self.param_groups):
            raise ValueError(f"{name}: betas and eps are shared by all parameter groups")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.nonfinite = nonfinite
        self.accumulation_steps = accumulation_steps
        self.divisor_slot = None   # an index into `aux`: the window's divisor is that device value, not the host's micro-step count
        self._micro = 0            # micro-steps taken in the open window
        ps = self.bucket_params()
        dev = ps[0].device
        self._check_params(ps, dev)
        align = 64  # every parameter view starts on a 256-byte boundary (16-byte vector loads in the cast / pack kernels)
        pad = lambda k: (k + align - 1) // align * align
        n = sum(pad(p.numel()) for p in ps)
        self._offsets = []       # one flat list over all groups, in bucket order
        self._group_first = []   # where each group starts in the bucket: a multiple of `align`
        self.flat_p = torch.zeros((n,), dtype=torch.float32, device=dev)
        # gradients + AUX_SLOTS trailing scalars (e.g. the rank's partial loss value) = ONE all-reduce message (`flat_comm`);
        # the optimizer kernel only ever sees the first n elements (`flat_g`)
        self.flat_comm = torch.zeros((n + self.AUX_SLOTS,), dtype=torch.float32, device=dev)
        self.flat_g = self.flat_comm[:n]
        self.aux = self.flat_comm[n:]
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        off = 0
        with torch.no_grad():
            for grp in self.param_groups:
                self._group_first.append(off)
                for p in grp["params"]:
                    k = p.numel()
                    self.flat_p[off : off + k].copy_(p.reshape(-1))
                    p.data = self.flat_p[off : off + k].view(p.shape)
                    p.grad = self.flat_g[off : off + k].view(p.shape)
                    self._offsets.append(off)
                    off += pad(k)
        self.step_count = 0
        self.grad_scale = 1.0  # e.g. 1/world_size after a SUM all-reduce (DDP's mean)
        # the device record of the norm launch (struct clibd_grad_record): norm and coefficient as fp32 bits, skip_now, skipped_total
        self._record = torch.zeros((4,), dtype=torch.int32, device=dev)
        self.grad_norm = self._record[0:1].view(torch.float32)
        self.skipped_steps = self._record[3:4]
        self._norm_ws = ops.grad_norm_workspace(n, dev)

    @staticmethod
    def _check_params(ps, dev):
        if not all(p.is_cuda and p.dtype == torch.float32 and p.device == dev for p in ps):
            raise ValueError("FusedAdamW: parameters must be fp32 tensors on one GPU")

    def bucket_params(self):
        """every parameter in bucket order (group after group): `_offsets[i]` is where `bucket_params()[i]` starts"""
        return [p for g in self.param_groups for p in g["params"]]

    @property
    def window_closes(self) -> bool:
        """True iff the next `step()` applies the update (always, with accumulation_steps=1)"""
        return self._micro + 1 >= self.accumulation_steps

    @property
    def window_open(self) -> bool:
        """True between the first `step()` of a window and the one that applies it"""
        return self._micro > 0

    @property
    def micro_steps(self) -> int:
        """micro-steps taken in the open window (0: none is open)"""
        return self._micro

    def zero_grad(self, set_to_none: bool = False):
        # gradients stay resident as views of the flat bucket (autograd accumulates in place); inside a window they are kept
        if self._micro == 0:
            self.flat_comm.zero_()
        for p, off in zip(self.bucket_params(), self._offsets):
            k = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * off:
                p.grad = self.flat_g[off : off + k].view(p.shape)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._micro += 1
        if self._micro >= self.accumulation_steps:
            self._apply()
        return loss

    @torch.no_grad()
    def flush(self) -> bool:
        """apply the open window although it holds fewer than accumulation_steps micro-steps; False (and no launch) when none is open"""
        if self._micro == 0:
            return False
        self._apply()
        return True

    def _apply(self):
        slot = self.divisor_slot
        if slot is not None and not 0 <= int(slot) < self.AUX_SLOTS:
            raise ValueError(f"{type(self).__name__}: divisor_slot must be in 0..{self.AUX_SLOTS - 1}")
        micro, self._micro = self._micro, 0
        g = self.param_groups[0]
        self.step_count += 1
        b1, b2 = g["betas"]
        skip = self.nonfinite == "skip"
        # the host's divisor: mean of the micro-batches' means.  micro == 1 leaves grad_scale as it is (x / 1), so k = 1 is what it was
        scale = self.grad_scale if slot is not None or micro == 1 else self.grad_scale / micro
        if slot is None and self.max_grad_norm is None and not skip and len(self.param_groups) == 1:
            self._update(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, g["lr"], b1, b2, g["eps"], g["weight_decay"],
                         self.step_count, scale)
            return
        record = None
        if slot is not None:
            record = self._record
            ops.grad_norm_div(self.flat_g, record, self._norm_ws, self.aux[int(slot) : int(slot) + 1], scale, self.max_grad_norm, skip)
        elif self.max_grad_norm is not None or skip:
            record = self._record
            ops.grad_norm(self.flat_g, record, self._norm_ws, scale, self.max_grad_norm, skip)
        table = [(first, grp["lr"], grp["weight_decay"]) for first, grp in zip(self._group_first, self.param_groups)]
        self._update_groups(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, table, b1, b2, g["eps"], self.step_count, scale, record)

    def _update(self, *args):
        ops.adamw_step(*args)

    def _update_groups(self, *args):
        ops.adamw_step_groups(*args)


class FusedAdam(FusedAdamW):
    """torch.optim.Adam(weight_decay=...) on the same flat bucket: the decay is L2 added to the gradient before the moments, not AdamW's
    decoupled shrink (the SimCLR pre-training's optimizer, reference scripts/unimodel/unimodel_training_for_image_encoder.py).
    Parameter groups, `max_grad_norm`, `nonfinite` and `accumulation_steps` as in FusedAdamW."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm: Optional[float] = None,
                 nonfinite: str = "propagate", accumulation_steps: int = 1):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, nonfinite=nonfinite,
                         accumulation_steps=accumulation_steps)

    def _update(self, *args):
        ops.adam_l2_step(*args)

    def _update_groups(self, *args):
        ops.adam_l2_step_groups(*args)


def refuse_windows_under_data_parallel(optimizer, who: str) -> None:
    """for drivers that all-reduce the flat bucket themselves, once per micro-step: with accumulation_steps > 1 the sum of the first
    micro-steps would be reduced again with every later one"""
    if getattr(optimizer, "accumulation_steps", 1) > 1:
        raise ValueError(f"{who}: accumulation_steps > 1 under world_size > 1: this driver all-reduces the gradient bucket at every step, and "
                         "a bucket reduced twice is silently wrong (clibd_amd.mlm reduces once per window)")


def decay_parameter_names(module: torch.nn.Module):
    """(names that take weight decay, names exempt from it) by HF Trainer's rule: parameters of nn.LayerNorm modules and every parameter
    whose name ends in `bias` are exempt.  Trainable parameters only; a tied weight appears once, under its first name."""
    in_ln = {id(p) for m in module.modules() if isinstance(m, torch.nn.LayerNorm) for p in m.parameters(recurse=False)}
    decay, exempt = [], []
    for name, p in module.named_parameters():   # removes duplicates: a tied parameter once
        if p.requires_grad:
            (exempt if id(p) in in_ln or name.endswith("bias") else decay).append(name)
    return decay, exempt


def decay_parameter_groups(module: torch.nn.Module, weight_decay: float):
    """Two parameter-group dicts for FusedAdamW / FusedAdam (or a torch optimizer): `decay_parameter_names`' first list with `weight_decay`,
    its second with 0.  An empty group is left out."""
    named = dict(module.named_parameters())
    decay, exempt = decay_parameter_names(module)
    groups = [{"params": [named[n] for n in decay], "weight_decay": float(weight_decay)},
              {"params": [named[n] for n in exempt], "weight_decay": 0.0}]
    return [g for g in groups if g["params"]]
