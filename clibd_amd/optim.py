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

Refused or not here: norm types other than 2, clipping by value, per-group betas or eps, amsgrad, maximize, more than 8 groups, LAMB and
LARS, gradient accumulation, a device-side step counter.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

MAX_GROUPS = 8  # CLIBD_OPTIM_MAX_GROUPS (include/clibd_hip_optim.h): the group table travels in the kernel arguments


class FusedAdamW(torch.optim.Optimizer):
    AUX_SLOTS = 64  # spare fp32 slots behind the gradients in the same allocation: scalars that ride along the gradient all-reduce

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm: Optional[float] = None,
                 nonfinite: str = "propagate"):
        name = type(self).__name__
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

    def zero_grad(self, set_to_none: bool = False):
        # gradients stay resident as views of the flat bucket (autograd accumulates in place)
        self.flat_comm.zero_()
        for p, off in zip(self.bucket_params(), self._offsets):
            k = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * off:
                p.grad = self.flat_g[off : off + k].view(p.shape)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        self.step_count += 1
        b1, b2 = g["betas"]
        skip = self.nonfinite == "skip"
        if self.max_grad_norm is None and not skip and len(self.param_groups) == 1:
            self._update(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, g["lr"], b1, b2, g["eps"], g["weight_decay"],
                         self.step_count, self.grad_scale)
            return loss
        record = None
        if self.max_grad_norm is not None or skip:
            record = self._record
            ops.grad_norm(self.flat_g, record, self._norm_ws, self.grad_scale, self.max_grad_norm, skip)
        table = [(first, grp["lr"], grp["weight_decay"]) for first, grp in zip(self._group_first, self.param_groups)]
        self._update_groups(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, table, b1, b2, g["eps"], self.step_count, self.grad_scale,
                            record)
        return loss

    def _update(self, *args):
        ops.adamw_step(*args)

    def _update_groups(self, *args):
        ops.adamw_step_groups(*args)


class FusedAdam(FusedAdamW):
    """torch.optim.Adam(weight_decay=...) on the same flat bucket: the decay is L2 added to the gradient before the moments, not AdamW's
    decoupled shrink (the SimCLR pre-training's optimizer, reference scripts/unimodel/unimodel_training_for_image_encoder.py).
    Parameter groups, `max_grad_norm` and `nonfinite` as in FusedAdamW."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm: Optional[float] = None,
                 nonfinite: str = "propagate"):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, nonfinite=nonfinite)

    def _update(self, *args):
        ops.adam_l2_step(*args)

    def _update_groups(self, *args):
        ops.adam_l2_step_groups(*args)


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
