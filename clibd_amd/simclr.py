"""SimCLR image-only pre-training: drop-in for `bioscanclip.util.simclr` and the two factory functions of
`bioscanclip.model.simple_clip` (reference util/simclr.py:16-168, model/simple_clip.py:64-97) on the MI355X HIP engine.

It produces the file `load_clip_model` consumes through `model_config.image.image_encoder_trained_with_simclr_style_ckpt_path`:
`{"epoch", "arch", "state_dict", "optimizer"}` with the timm keys of the ViT under the `module.` prefix of the reference's
DDP-wrapped model, so files travel in both directions.

The ViT runs through `clibd_amd.towers.ViTTower` under full fine-tuning (bf16 GEMM operands, fp32 accumulation, statistics and
master weights: there is no fp16 GradScaler path, no wandb and no tensorboard); the loss is the fused NT-Xent kernel
(csrc/ntxent.hip, no N x N matrix in memory) and the optimizer `clibd_amd.optim.FusedAdam` (torch.optim.Adam with coupled L2).
A step takes the two view tensors, as the contrastive step takes images, or a packed batch of decoded pixels with one record per
view (`clibd_amd.simclr_views.pack_two_views` / `collate_two_views`): the view augmentations of the reference's data pipeline (crop,
flip, colour jitter, grayscale, blur) then run on the device (csrc/views.hip) and feed the tower directly.
"""
from __future__ import annotations

import os
import shutil
from typing import Optional

import torch
import torch.nn as nn

from . import ops, simclr_views
from .chunked import ReplayGuard, two_pass, validate_chunk_size
from .engine import NotSupportedYet
from .model.image_encoder import create_vit
from .model.simple_clip import SimpleCLIP, _get
from .towers import ViTTower

F32 = torch.float32


class SimCLRViT(nn.Module):
    """A timm-shaped ViT with its 1000-wide classifier head as the SimCLR projection (the reference trains
    `timm.create_model(name, pretrained=True)` as it comes).  forward(images [B,3,224,224]) -> [B, num_classes] on the HIP
    tower; `state_dict()` keys are `module.<timm key>`, what the reference's DistributedDataParallel wrapper saves."""

    def __init__(self, vit):
        super().__init__()
        self.module = vit
        self._tower = None

    def tower(self) -> ViTTower:
        if self._tower is None:
            self._tower = ViTTower(self.module, {})
        return self._tower

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        return self.tower()(images)


def load_vit_for_simclr_training(args, device=None):
    """reference simple_clip.py:64-72: the ViT named by `model_config.image.pre_train_model` (default vit_base_patch16_224) with its
    1000-class head, every parameter trainable.  Pretrained weights come from the LOCAL `model_config.image.vit_checkpoint` only (a timm
    state dict, or {"state_dict": ...} with or without the `module.` prefix); without it the initialisation is random."""
    image_cfg = _get(args.model_config, "image")
    name = _get(image_cfg, "pre_train_model", "vit_base_patch16_224") if image_cfg is not None else "vit_base_patch16_224"
    vit = create_vit(name, num_classes=1000)
    ck = _get(image_cfg, "vit_checkpoint") if image_cfg is not None else None
    if ck:
        sd = torch.load(ck, map_location="cpu", weights_only=False)
        sd = sd.get("state_dict", sd)
        vit.load_state_dict({k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}, strict=False)
    model = SimCLRViT(vit)
    if device is not None:
        model.to(device)
    for p in model.parameters():
        p.requires_grad = True
    return model


def wrap_vit_into_simple_clip(args, vit, device=None):
    """reference simple_clip.py:75-97: a SimpleCLIP with the image tower only, everything trainable.  `vit` is the model of
    `load_vit_for_simclr_training` (or a bare timm-shaped ViT, which is wrapped the same way)."""
    image_encoder = vit if isinstance(vit, SimCLRViT) else SimCLRViT(vit)
    model = SimpleCLIP(image_encoder=image_encoder, dna_encoder=None, language_encoder=None)
    if device is not None:
        model.to(device)
    for p in model.parameters():
        p.requires_grad = True
    return model


class _NTXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, owner):
        f = features.detach().to(F32).contiguous()
        ws = owner._workspace(f)
        loss = torch.empty((1,), dtype=F32, device=f.device)
        ops.ntxent_fwd(f, owner.inv_temperature, loss, ws, owner.last_top1)
        owner._generation += 1
        ctx.save_for_backward(f)
        ctx.owner, ctx.ws, ctx.generation, ctx.dtype = owner, ws, owner._generation, features.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (f,) = ctx.saved_tensors
        owner = ctx.owner
        if ctx.generation != owner._generation:
            # another forward has used the workspace since: restore this call's row statistics
            ops.ntxent_fwd(f, owner.inv_temperature, torch.empty((1,), dtype=F32, device=f.device), ctx.ws, None)
            owner._generation += 1
            ctx.generation = owner._generation
        df = torch.empty_like(f)
        ops.ntxent_bwd(f, owner.inv_temperature, df, ctx.ws, dloss.detach().to(F32).reshape(1).contiguous())
        return df.to(ctx.dtype), None


class NTXentLoss(nn.Module):
    """`CrossEntropyLoss()(*info_nce_loss(features))` of the reference (util/simclr.py:64-92, 118-119) as one fused loss:
    features [2b, D] hold view 1 of the b samples, then view 2; rows are normalised inside the kernel.  `last_top1` is a device
    int32 scalar with the top-1 hit count of the last forward (the reference's `accuracy(logits, labels)`, as a count)."""

    def __init__(self, temperature: float = 0.07, n_views: int = 2):
        super().__init__()
        if n_views != 2:
            raise NotSupportedYet("NTXentLoss: n_views must be 2 (the only value the reference's configs ship)")
        if not temperature > 0:
            raise ValueError("NTXentLoss: temperature must be positive")
        self.temperature = float(temperature)
        self.inv_temperature = 1.0 / float(temperature)
        self.last_top1: Optional[torch.Tensor] = None
        self._ws = {}
        self._generation = 0

    def _workspace(self, f):
        key = (f.device, tuple(f.shape))
        if key not in self._ws:
            self._ws = {key: ops.ntxent_workspace(f.shape[0], f.shape[1], f.device)}
        if self.last_top1 is None or self.last_top1.device != f.device:
            self.last_top1 = torch.zeros((1,), dtype=torch.int32, device=f.device)
        return self._ws[key]

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        if features.dim() != 2 or features.shape[0] % 2 != 0 or features.shape[0] < 4:
            raise ValueError("NTXentLoss: expected [2b, D] features with b >= 2")
        return _NTXentFn.apply(features, self)


def save_checkpoint(args, state, is_best, filename="checkpoint.pth.tar", ckpt_dir=None):
    """reference util/simclr.py:16-23; `ckpt_dir` overrides the reference's <project_root_path>/ckpt/uni_model/uni_model/image/<name>."""
    if ckpt_dir is None:
        ckpt_dir = os.path.join(args.project_root_path, "ckpt", "uni_model", "uni_model", "image", args.model_config.model_output_name)
    os.makedirs(ckpt_dir, exist_ok=True)
    torch.save(state, os.path.join(ckpt_dir, filename))
    if is_best:
        shutil.copyfile(os.path.join(ckpt_dir, filename), os.path.join(ckpt_dir, "model_best.pth.tar"))
    return ckpt_dir


class SimCLR(object):
    """reference util/simclr.py:50-168.  `model`: load_vit_for_simclr_training's module; `optimizer`: clibd_amd.optim.FusedAdam over
    its parameters (any torch optimizer works, the fused one also takes the tower's gradients straight into its flat bucket);
    `scheduler`: e.g. CosineAnnealingLR, stepped per epoch from epoch 2 as the reference does.

    Arithmetic: bf16 GEMM operands with fp32 accumulation, fp32 statistics, fp32 master weights and optimizer state, where the
    reference runs fp16 autocast with a GradScaler; there is no wandb / tensorboard logging.
    world_size > 1: like the reference, every rank computes the loss over its own 2b rows (no gather) and the gradients are averaged,
    here through one all-reduce of the optimizer's flat bucket (unmeasured on more than one GPU); that all-reduce runs at every step,
    so an optimizer with accumulation_steps > 1 raises ValueError there.  On one GPU such an optimizer accumulates the NT-Xent gradients
    of k steps (mean of means), which is NOT the loss of the k-times larger batch: a micro-batch's negatives are its own.
    chunk_size=c (keyword, default None = the plain step): `train_step` takes the two-pass chunked step of clibd_amd.chunked
    over row ranges of c of the 2b views — one NTXentLoss over all 2b rows, `last_top1` of the full batch, the exact gradient of the plain
    step with the activations of c rows in memory.  `replay_mismatch` is the replay guard's device counter (replay_guard=False: none)."""

    def __init__(self, *args, **kwargs):
        self.chunk_size = validate_chunk_size(kwargs.get("chunk_size"), "SimCLR")
        self._want_guard, self._guard = bool(kwargs.get("replay_guard", True)) and self.chunk_size is not None, None
        self.args = kwargs["args"]
        self.device = kwargs["device"]
        self.model = kwargs["model"].to(self.device)
        self.optimizer = kwargs["optimizer"]
        self.scheduler = kwargs.get("scheduler")
        mc = self.args.model_config
        self.criterion = NTXentLoss(temperature=mc.temperature, n_views=_get(mc, "n_views", 2))
        self._dist = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        if hasattr(self.optimizer, "flat_g"):
            if self._dist:
                from .optim import refuse_windows_under_data_parallel

                refuse_windows_under_data_parallel(self.optimizer, "SimCLR")
                self.optimizer.grad_scale = 1.0 / torch.distributed.get_world_size()   # SUM all-reduce, then DDP's mean
            if hasattr(self.model, "tower"):
                self.model.tower().grad_sink = {id(p): p.grad for p in self.optimizer.bucket_params()}
        elif self._dist:
            raise NotSupportedYet("SimCLR: data-parallel training needs clibd_amd.optim.FusedAdam (the flat gradient bucket is the all-reduce message)")

    @property
    def replay_mismatch(self):
        """device int64 [1]: cached feature words the chunked steps' second pass did not reproduce (None without the guard)"""
        return None if self._guard is None else self._guard.mismatch

    def info_nce_loss(self, features):
        """Kept for callers of the reference's method, but returns the LOSS: the reference's (logits, labels) pair — the [2b, 2b-1]
        matrix with the positive moved to column 0 — is never formed.  `self.criterion.last_top1` holds the top-1 hit count."""
        return self.criterion(features)

    def train_step(self, images_1, images_2=None):
        """cat -> forward -> NT-Xent -> backward -> optimizer step; returns the device loss.  No host synchronisation.
        `images_1` alone may be a packed batch (`simclr_views.pack_two_views`): its 2b views are generated on the device, first views
        then second views, and there is no cat."""
        if simclr_views.is_packed(images_1):
            if images_2 is not None:
                raise ValueError("SimCLR.train_step: a packed batch holds both views")
            images = simclr_views.apply(images_1, self.device)
        else:
            images = torch.cat([images_1, images_2], dim=0).to(self.device)
        self.optimizer.zero_grad()
        if self.chunk_size is not None:
            if self._guard is None and self._want_guard:
                self._guard = ReplayGuard(images.device)
            towers = [self.model.tower()] if hasattr(self.model, "tower") else []
            loss, _ = two_pass(lambda x: (self.model(x),), (images,), self.chunk_size, lambda leaves: self.info_nce_loss(leaves[0]),
                               towers=towers, guard=self._guard)
        else:
            features = self.model(images)
            loss = self.info_nce_loss(features)
            loss.backward()
        if self._dist:
            torch.distributed.all_reduce(self.optimizer.flat_comm)
        self.optimizer.step()
        return loss.detach()

    def train(self, train_loader, rank=0, ckpt_dir=None):
        mc = self.args.model_config
        self.model.train()
        if rank == 0:
            print(f"Start SimCLR training for {mc.epochs} epochs.")
        best_loss = None
        for epoch_counter in range(mc.epochs):
            running = torch.zeros((), dtype=F32, device=self.device)
            hits = torch.zeros((), dtype=torch.int64, device=self.device)
            n = rows = 0
            for batch in train_loader:           # (images_1, images_2), or a packed batch of both views
                if simclr_views.is_packed(batch):
                    running += self.train_step(batch)
                    rows += batch["xforms"].shape[0]
                else:
                    images_1, images_2 = batch
                    running += self.train_step(images_1, images_2)
                    rows += 2 * images_1.shape[0]
                hits += self.criterion.last_top1[0]
                n += 1
            epoch_loss_avg, nhits = torch.stack([running / max(n, 1), hits.to(F32)]).tolist()   # the one host fetch of the epoch
            top1 = 100.0 * nhits / max(rows, 1)
            # warmup for the first epochs (reference util/simclr.py:144-146)
            if epoch_counter >= 2 and self.scheduler is not None:
                self.scheduler.step()
            if rank == 0:
                print(f"Epoch: {epoch_counter}\tLoss: {epoch_loss_avg:.4f}\tTop1 accuracy: {top1:.2f}")
            is_best = best_loss is None or epoch_loss_avg < best_loss
            if is_best:
                best_loss = epoch_loss_avg
            if rank == 0:
                image_cfg = _get(mc, "image")
                arch = _get(image_cfg, "pre_train_model", "vit_base_patch16_224") if image_cfg is not None else "vit_base_patch16_224"
                save_checkpoint(self.args, {"epoch": mc.epochs, "arch": arch, "state_dict": {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                                            "optimizer": self.optimizer.state_dict()},
                                is_best=is_best, filename="checkpoint_{:04d}.pth.tar".format(mc.epochs), ckpt_dir=ckpt_dir)
        if rank == 0:
            print("Training has finished.")
        return best_loss
