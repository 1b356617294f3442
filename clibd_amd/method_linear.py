"""Seen/unseen classification by a linear-probe classifier (the reference's scripts/method_linear.py) on the device.

A copy of the image encoder gets a `Linear(output_dim, n_seen_species)` head and is fine-tuned under cross-entropy on the seen species.
A query's j-th prediction then comes from the classifier (source A: the class with the j-th largest softmax confidence) if that
confidence exceeds a threshold, and from the image -> DNA search over the unseen keys (source B) otherwise.  The threshold maximises the
harmonic mean of the seen and the unseen split's top-1 species accuracy over np.linspace(0, 1, 1001); micro / macro / per-class accuracy
of the merged predictions are reported at it.

The head's arithmetic is its own (include/clibd_hip_classifier.h): confidences are compared with `>` against the grid and
class indices are scored under `==`, so the head's product runs on split-bf16 operands (fp32-grade), the cross-entropy and the softmax
top-k in fp32, all in fixed summation orders.  What follows the two sources is method_nn's: clibd_threshold_sweep_hits,
clibd_threshold_merge, clibd_topk_label_hits and the reference's float64 arithmetic restated on integer counts.  Two conventions, as in
clibd_amd.method_nn: the reference's lists (function names and signatures of scripts/method_linear.py) and device tensors
(`classifier_seen_unseen_from_features`, `classifier_topk`).

Stated divergences:
  - the head has `num_classes` = the size of the label map by default (the reference hard-codes 916);
  - `build_image_classifier` trains what the copy's tower can differentiate — under LoRA the adapters, the projection head and the new
    layer, with the base weights frozen as in the contrastive training; everything under `disable_lora` — where the reference sets
    requires_grad on every parameter; `train_encoder=False` is the strict linear probe (the encoder runs without gradient);
  - `CrossEntropyLoss` is nn.CrossEntropyLoss() with its defaults only: class weights, label smoothing, another reduction or a
    non-default ignore_index raise NotSupportedYet, and a target outside [0, C) — the default ignore_index -100 included — contributes
    nothing while the divisor stays B, and sets bit 0 of `ops.ce_error_word` instead of raising (no host synchronisation in a step);
  - the epoch loss is accumulated on the device in fp32 and fetched once per epoch (the reference: a float64 mean of per-step `.item()`s);
  - `evaluate_epoch` takes its top-k class indices from clibd_softmax_topk (the reference: torch.argsort of the logits; the same
    indices unless two logits of a row are equal, where the lower index comes first here) and at most 8 of them;
  - each loader is embedded once per model (the reference embeds the queries once per key loader as well);
  - the optimizer is clibd_amd.optim.FusedAdamW (torch.optim.AdamW's update on one flat bucket), `last.pth` holds CPU tensors;
  - a `k_list` without 1 is a ValueError (the reference: KeyError), as in method_nn; no tqdm bar, hydra, wandb or CSV output."""
from __future__ import annotations

import copy
import os
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import eval as E
from . import method_nn as NN
from . import ops
from .engine import NotSupportedYet
from .method_nn import (check_for_acc_about_correct_predict_seen_or_unseen, choose_threshold, decide_prediction_with_threshold,  # noqa: F401
                        get_final_pred_and_acc, harmonic_mean, make_final_pred, print_acc_for_google_doc)

F32 = torch.float32
MAX_K = 5   # the reference's torch.topk(..., k=5) and make_prediction(max_k=5)


def threshold_grid(num_intervals: int = 1000) -> np.ndarray:
    """np.linspace(0, 1, num_intervals + 1) (scripts/method_linear.py:176): 1 001 points, one more than method_nn's grid"""
    return np.linspace(0, 1, num_intervals + 1)


# ============================================================================================================ autograd bridges
class _LinearF32Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.detach().to(F32).contiguous()
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return ops.linear_f32_fwd(x, weight.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        need_dx, need_dw, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx, dw, db = ops.linear_f32_bwd(dout.detach().to(F32).contiguous(), x, weight.detach(), need_dx, need_dw, need_db)
        return dx, dw, db


def linear_f32(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear(x, weight, bias) for fp32 [B, D] features at split-bf16 accuracy, differentiable (clibd_linear_f32_fwd / _bwd)"""
    return _LinearF32Fn.apply(x, weight, bias)


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        logits = logits.detach().to(F32)
        if logits.stride(-1) != 1:
            logits = logits.contiguous()
        loss, lse = ops.ce_rows_fwd(logits, target)
        ctx.save_for_backward(logits, target, lse)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        return ops.ce_rows_bwd(logits, target, lse, dloss.detach().to(F32).reshape(1).contiguous()), None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() — mean reduction, integer class targets — over fp32 logits [B, C] on the device, as one fused forward
    (one wave per row, online max and sum) and one fused backward.  See the module docstring for what is not supported."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean", label_smoothing: float = 0.0):
        super().__init__()
        if weight is not None:
            raise NotSupportedYet("CrossEntropyLoss: class weights")
        if label_smoothing != 0.0:
            raise NotSupportedYet("CrossEntropyLoss: label smoothing")
        if ignore_index != -100:
            raise NotSupportedYet("CrossEntropyLoss: a non-default ignore_index")
        if reduction != "mean" or size_average is not None or reduce is not None:
            raise NotSupportedYet("CrossEntropyLoss: only the mean reduction")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if input.dim() != 2 or target.dim() != 1 or target.dtype != torch.int64:
            raise NotSupportedYet("CrossEntropyLoss: expected logits [B, C] and int64 class targets [B]")
        return _CrossEntropyFn.apply(input, target.to(input.device))


# ==================================================================================================================== the model
class ViTWIthExtraLayer(nn.Module):
    """scripts/method_linear.py:26-39 (the reference's spelling).  `vit_model`: any module that returns device fp32 [B, D] features;
    `new_linear_layer`: an nn.Linear used as a parameter holder — its product is clibd_linear_f32_fwd, its backward
    clibd_linear_f32_bwd.  State-dict keys: vit.*, new_linear_layer.weight, new_linear_layer.bias, as in the reference's last.pth.
    `train_encoder=False`: the encoder runs under no_grad (the strict linear probe)."""

    def __init__(self, vit_model, new_linear_layer, train_encoder: bool = True):
        super(ViTWIthExtraLayer, self).__init__()
        self.vit = vit_model
        self.new_linear_layer = new_linear_layer
        self.train_encoder = bool(train_encoder)

    def get_feature(self, x):
        return self.vit(x)

    def forward(self, x):
        if self.train_encoder:
            outputs = self.vit(x)
        else:
            with torch.no_grad():
                outputs = self.vit(x)
        return linear_f32(outputs, self.new_linear_layer.weight, self.new_linear_layer.bias)


def build_image_classifier(original_model, num_classes: int, train_encoder: bool = True, output_dim: Optional[int] = None) -> ViTWIthExtraLayer:
    """scripts/method_linear.py:473-481: a deep copy of `original_model.image_encoder` (its cached tower dropped: the copy builds its
    own over the copied weights) with a new Linear(output_dim, num_classes) on top.  num_classes: the size of the label map (the
    reference: 916).  The copy keeps the requires_grad flags of the original — what its tower differentiates, see the module
    docstring; with train_encoder=False every encoder parameter is frozen and only the head trains."""
    src = original_model.image_encoder
    if src is None:
        raise ValueError("build_image_classifier: the model has no image encoder")
    cached = src.__dict__.get("_tower", None)
    try:
        if cached is not None:
            src._tower = None
        enc = copy.deepcopy(src)
    finally:
        if cached is not None:
            src._tower = cached
    if output_dim is None:
        for base in (getattr(enc, "base_image_encoder", None), getattr(enc, "module", None), enc):   # CLIBDImageEncoder, SimCLRViT, a bare ViT
            output_dim = getattr(getattr(base, "head", None), "out_features", None) or getattr(base, "num_classes", None)
            if output_dim:
                break
        if not output_dim:
            raise ValueError("build_image_classifier: pass output_dim= (the encoder does not tell its feature width)")
    dev = next(enc.parameters()).device
    head = nn.Linear(int(output_dim), int(num_classes)).to(dev)
    if not train_encoder:
        for p in enc.parameters():
            p.requires_grad = False
    return ViTWIthExtraLayer(enc, head, train_encoder=train_encoder)


# ================================================================================================================= host helpers
def get_all_unique_species_from_dataloader(dataloader):
    all_species = []
    for batch in dataloader:
        label_batch = batch[6]
        all_species = all_species + list(label_batch["species"])
    return list(set(all_species))


def load_all_seen_species_name_and_create_label_map(train_seen_dataloader):
    """scripts/method_linear.py:286-313: ({species: class index}, {class index: {species, order, family, genus}}), the species sorted;
    the other levels are those of a species' first appearance."""
    all_seen_species = []
    species_to_other_labels = {}
    for batch in train_seen_dataloader:
        label_batch = batch[6]
        all_seen_species = all_seen_species + list(label_batch["species"])
        for curr_idx in range(len(label_batch["species"])):
            sp = label_batch["species"][curr_idx]
            if sp not in species_to_other_labels:
                species_to_other_labels[sp] = {"order": label_batch["order"][curr_idx], "family": label_batch["family"][curr_idx],
                                               "genus": label_batch["genus"][curr_idx]}
    all_seen_species = list(set(all_seen_species))
    all_seen_species.sort()
    label_to_index_dict, idx_to_all_labels = {}, {}
    for idx, species_label in enumerate(all_seen_species):
        label_to_index_dict[species_label] = idx
        other = species_to_other_labels[species_label]
        idx_to_all_labels[idx] = {"species": species_label, "order": other["order"], "family": other["family"], "genus": other["genus"]}
    return label_to_index_dict, idx_to_all_labels


def label_to_index(label, label_map):
    return label_map[label]


def label_batch_to_species_idx(label_batch, species_level_label_to_index_dict):
    """int64 [B] class indices of a batch's species; an unknown species is a KeyError, as in the reference"""
    return torch.tensor([label_to_index(species, species_level_label_to_index_dict) for species in label_batch["species"]], dtype=torch.int64)


def _class_labels(idx_to_all_labels) -> List[dict]:
    n = len(idx_to_all_labels)
    try:
        return [idx_to_all_labels[i] for i in range(n)]
    except (KeyError, IndexError):
        raise ValueError("method_linear: idx_to_all_labels must map every class index 0 .. C - 1") from None


def _images(image_input_batch, device):
    from . import augment

    return augment.apply(image_input_batch, device) if augment.is_packed(image_input_batch) else image_input_batch.to(device)


# ================================================================================================================ training loop
def evaluate_epoch(model, dataloader, device, species_level_label_to_index_dict, k_values=None):
    """scripts/method_linear.py:349-383: {"top{k}_accuracy": the fraction of samples whose class is among the k most confident}.  The
    class indices come from clibd_softmax_topk, the hits are counted by clibd_topk_label_hits on a one-level table (class index ->
    itself); hits / N is what np.mean of the reference's boolean array is.  Leaves the model in eval mode, as the reference does."""
    if k_values is None:
        k_values = [1, 3, 5]
    ks = sorted({int(k) for k in k_values})
    if not ks or ks[0] < 1 or ks[-1] > 8:
        raise ValueError("evaluate_epoch: k_values must lie in 1..8")
    model.eval()
    dev = torch.device(device)
    idx_all, targets = [], []
    n_classes = len(species_level_label_to_index_dict)
    with torch.no_grad():
        for batch in dataloader:
            targets.append(label_batch_to_species_idx(batch[6], species_level_label_to_index_dict))
            output = model(_images(batch[1], dev))
            n_classes = max(n_classes, output.shape[1])
            idx_all.append(ops.softmax_topk(output, min(ks[-1], output.shape[1]))[1])
    idx = torch.cat(idx_all, dim=0)
    target = torch.cat(targets).to(torch.int32).reshape(-1, 1).to(dev)
    N, m = idx.shape
    table = torch.arange(n_classes, dtype=torch.int32, device=dev).reshape(-1, 1)
    kk = sorted({min(k, m) for k in ks})
    _, lh, _, _ = ops.topk_label_hits(idx, table, target, [0, n_classes], kk)
    lh = lh.cpu().numpy()[0, :, 0]
    return {f"top{k}_accuracy": np.float64(int(lh[kk.index(min(int(k), m))])) / N for k in k_values}


def fine_tuning_epoch(args, model, train_dataloader, val_seen_dataloader, val_unseen_dataloader, optimizer, criterion, scheduler, device,
                      species_level_label_to_index_dict, step_losses: Optional[list] = None):
    """scripts/method_linear.py:322-346: one pass over the training loader, then `evaluate_epoch` on the seen validation loader (skipped
    when it is None).  No host synchronisation inside a step: the loss is accumulated on the device and fetched once, as SimCLR.train
    does; `step_losses` (a list) receives every step's device loss.  Returns (epoch_loss, seen_evaluation_result)."""
    dev = torch.device(device)
    running = torch.zeros((), dtype=F32, device=dev)
    n = 0
    for batch in train_dataloader:
        target = label_batch_to_species_idx(batch[6], species_level_label_to_index_dict).to(dev)
        optimizer.zero_grad()
        output = model(_images(batch[1], dev))
        loss = criterion(output, target)
        loss.backward()
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        running += loss.detach()
        if step_losses is not None:
            step_losses.append(loss.detach())
        n += 1
    epoch_loss = float(running.item()) / max(n, 1)          # the one host fetch of the epoch
    seen_evaluation_result = None
    if val_seen_dataloader is not None:
        print("Eval on seen val.")
        seen_evaluation_result = evaluate_epoch(model, val_seen_dataloader, device, species_level_label_to_index_dict)
        print("Evaluation Result:", seen_evaluation_result)
    return epoch_loss, seen_evaluation_result


def _cfg(args, name, default=None):
    node = getattr(getattr(args, "model_config", None), "fine_tuning_set", None)
    if node is None:
        return default
    return node.get(name, default) if isinstance(node, dict) else getattr(node, name, default)


def train_image_classifier(args, image_classifier, train_seen_dataloader, seen_val_dataloader, unseen_val_dataloader, device,
                           species_level_label_to_index_dict, epochs: Optional[int] = None, output_dir: Optional[str] = None,
                           save_ckpt: Optional[bool] = None):
    """The training block of the reference's main (scripts/method_linear.py:487-528).  `<output_dir>/last.pth` present: it is loaded,
    every parameter is frozen and nothing trains.  Otherwise FusedAdamW(lr=1e-4) + OneCycleLR(max_lr=1e-4, total_steps = steps x epochs)
    under `CrossEntropyLoss`, `fine_tuning_epoch` per epoch, and — with save_ckpt — the state dict written to last.pth after every epoch.
    epochs / output_dir / save_ckpt default to args.model_config.fine_tuning_set.{epochs, fine_tune_model_output_dir} and args.save_ckpt.
    Returns {"loaded": bool, "epoch_losses": [...], "evaluation": [...], "last_ckpt_path": path}."""
    from torch.optim.lr_scheduler import OneCycleLR

    from .optim import FusedAdamW

    epochs = int(_cfg(args, "epochs") if epochs is None else epochs)
    output_dir = _cfg(args, "fine_tune_model_output_dir") if output_dir is None else output_dir
    save_ckpt = bool(getattr(args, "save_ckpt", False)) if save_ckpt is None else bool(save_ckpt)
    last_ckpt_path = os.path.join(output_dir, "last.pth")
    os.makedirs(output_dir, exist_ok=True)
    out = {"loaded": False, "epoch_losses": [], "evaluation": [], "last_ckpt_path": last_ckpt_path}
    image_classifier.to(device)
    if os.path.exists(last_ckpt_path):
        print(f"Found pre-trained model in {last_ckpt_path}")
        image_classifier.load_state_dict(torch.load(last_ckpt_path, map_location=device))
        for param in image_classifier.parameters():
            param.requires_grad = False
        out["loaded"] = True
        return out
    criterion = CrossEntropyLoss()
    optimizer = FusedAdamW(image_classifier.parameters(), lr=0.0001)
    total_steps = len(train_seen_dataloader) * epochs
    scheduler = OneCycleLR(optimizer, max_lr=0.0001, total_steps=total_steps)

    def save():
        torch.save({k: v.detach().cpu().clone() for k, v in image_classifier.state_dict().items()}, last_ckpt_path)
        print(f"Last ckpt: {last_ckpt_path}")

    for epoch in range(epochs):
        epoch_loss, seen_evaluation_result = fine_tuning_epoch(args, image_classifier, train_seen_dataloader, seen_val_dataloader, unseen_val_dataloader,
                                                               optimizer, criterion, scheduler, device, species_level_label_to_index_dict)
        out["epoch_losses"].append(epoch_loss)
        out["evaluation"].append(seen_evaluation_result)
        if save_ckpt:
            save()
    return out


# =============================================================================================================== source A: lists
def classifier_topk(image_encoder, dataloader, device, k: int = MAX_K):
    """The device form of `inference_with_fine_tuned_image_encoder`: (conf fp32 [N, k], idx int64 [N, k]) of
    torch.topk(F.softmax(image_encoder(images), -1), k) over the loader, on the GPU, and the ground-truth label list."""
    dev = torch.device(device)
    conf, idx, gt_labels = [], [], []
    with torch.no_grad():
        for batch in dataloader:
            c, i = ops.softmax_topk(image_encoder(_images(batch[1], dev)), k)
            conf.append(c)
            idx.append(i)
            gt_labels.extend(E.convert_label_dict_to_list_of_dict(batch[6]))
    return torch.cat(conf, dim=0), torch.cat(idx, dim=0), gt_labels


def inference_with_fine_tuned_image_encoder(image_encoder, dataloader, species_level_label_to_index_dict, idx_to_all_labels, device):
    """scripts/method_linear.py:42-86: (confidences [N][5] as Python floats of the fp32 values, predicted labels [{level: [5 labels]}],
    ground-truth labels).  One copy to the host at the end."""
    conf, idx, gt_labels = classifier_topk(image_encoder, dataloader, device, MAX_K)
    labels = _class_labels(idx_to_all_labels)
    pred_labels = [{level: [labels[i][level] for i in row] for level in labels[0].keys()} for row in idx.cpu().numpy().tolist()]
    return conf.cpu().numpy().tolist(), pred_labels, gt_labels


def inference_with_original_image_encoder_and_dna_encoder(original_model, seen_dataloader, unseen_dataloader, val_unseen_keys_dataloader,
                                                          test_unseen_keys_dataloader, device):
    """scripts/method_linear.py:128-160: the image -> DNA predictions of both query loaders over the val + test unseen keys"""
    sp, _, _, up, _, _ = NN.inference_with_original_image_encoder_and_dna_encoder(original_model, seen_dataloader, unseen_dataloader,
                                                                                  [val_unseen_keys_dataloader, test_unseen_keys_dataloader], device, key_type="dna")
    return sp, up


def search_threshold_with_harmonic_mean(args, all_split_data, num_intervals=1000, k_list=None):
    """scripts/method_linear.py:175-200: method_nn's search on np.linspace(0, 1, num_intervals + 1)"""
    return NN.search_threshold_with_harmonic_mean(args, all_split_data, thresholds=threshold_grid(num_intervals), k_list=k_list)


def sweep_top1_hits(all_split_data, num_intervals=1000) -> np.ndarray:
    """int [num_intervals + 1, n_splits]: the species top-1 hit counts of the merged predictions at every threshold of the grid"""
    return NN.sweep_top1_hits(all_split_data, threshold_grid(num_intervals))


# ============================================================================================================== device convention
def classifier_seen_unseen_from_features(seen_logits, unseen_logits, class_labels, seen_query, unseen_query, unseen_keys, unseen_keys_label,
                                         seen_gt, unseen_gt, k_list, searched_threshold=None, thresholds=None, with_predictions=True,
                                         num_intervals=1000, max_k=MAX_K):
    """method_2_inference_and_eval_for_seen_and_unseen from device tensors.  Source A: the classifier's logits fp32 [Q, C] of both splits
    (clibd_softmax_topk gives conf and class indices; `class_labels`: [{level: label}] per class, the key table [C, 4]).  Source B: the
    image features of the ORIGINAL encoder searched against the unseen keys' DNA features (a tensor, numpy array or prepared KeyBank).
    Then method_nn.seen_unseen_from_sources on np.linspace(0, 1, num_intervals + 1) (or `thresholds`).  Returns the reference's
    (seen_output_dict, unseen_output_dict); with_predictions=False stores merged int64 indices into class_labels + unseen_keys_label."""
    ks = E._check_k_list(list(k_list))
    if searched_threshold is None and 1 not in ks:
        raise ValueError("method_linear: the threshold search reads the top-1 accuracy, k_list must contain 1")
    m = max(int(max_k), ks[-1])
    if m > 8:
        raise ValueError("method_linear: at most 8 predictions per query")
    dev = seen_logits.device
    Qs, Qu = len(seen_gt), len(unseen_gt)
    logits = torch.cat([seen_logits, unseen_logits], dim=0).to(F32)
    queries = torch.cat([E._as_device(seen_query, dev), E._as_device(unseen_query, dev)], dim=0)
    if logits.shape[0] != Qs + Qu or queries.shape[0] != Qs + Qu or Qs == 0 or Qu == 0:
        raise ValueError("method_linear: one ground-truth label per query, and both splits non-empty")
    bank_b, Nkb = NN._prepared(unseen_keys, dev)
    if logits.shape[1] != len(class_labels) or Nkb != len(unseen_keys_label) or min(logits.shape[1], Nkb) < m:
        raise ValueError(f"method_linear: one label per class and per key, and at least {m} of each")
    conf, idx_a = ops.softmax_topk(logits, m)
    _, idx_b = E.topk_search(queries, bank_b, m, cache=False)
    grid = None
    if searched_threshold is None:
        grid = threshold_grid(num_intervals) if thresholds is None else NN._grid(num_intervals, thresholds)
    return NN.seen_unseen_from_sources(conf, idx_a, idx_b, class_labels, unseen_keys_label, seen_gt, unseen_gt, ks, searched_threshold, grid,
                                       with_predictions)


def _logits_of(image_classifier, dataloader, dev):
    out, gt = [], []
    with torch.no_grad():
        for batch in dataloader:
            out.append(image_classifier(_images(batch[1], dev)))
            gt.extend(E.convert_label_dict_to_list_of_dict(batch[6]))
    return torch.cat(out, dim=0), gt


def method_2_inference_and_eval_for_seen_and_unseen(args, image_classifier, original_model, seen_dataloader, unseen_dataloader,
                                                    val_unseen_keys_dataloader, test_unseen_keys_dataloader, species_level_label_to_index_dict,
                                                    idx_to_all_labels, device, searched_threshold=None, k_list=None, with_predictions=True):
    """scripts/method_linear.py:220-275.  Every loader is embedded ONCE per model and stays on the device: the classifier's logits and the
    original encoder's image features of the two query loaders, the DNA features of the val + test unseen keys (concatenated), then
    `classifier_seen_unseen_from_features`."""
    ks = NN._k_list_of(args, k_list)
    dev = torch.device(device)
    image_classifier.eval()
    seen_logits, _ = _logits_of(image_classifier, seen_dataloader, dev)
    unseen_logits, _ = _logits_of(image_classifier, unseen_dataloader, dev)
    _, seen_q, _, _, seen_gt = E.get_feature_and_label(seen_dataloader, original_model, device, as_numpy=False)
    _, unseen_q, _, _, unseen_gt = E.get_feature_and_label(unseen_dataloader, original_model, device, as_numpy=False)
    _, _, val_k, _, val_k_label = E.get_feature_and_label(val_unseen_keys_dataloader, original_model, device, as_numpy=False)
    _, _, test_k, _, test_k_label = E.get_feature_and_label(test_unseen_keys_dataloader, original_model, device, as_numpy=False)
    if seen_q is None or unseen_q is None or val_k is None or test_k is None:
        raise ValueError("method_linear: the original model needs an image and a DNA encoder")
    return classifier_seen_unseen_from_features(seen_logits, unseen_logits, _class_labels(idx_to_all_labels), seen_q, unseen_q,
                                                torch.cat([val_k, test_k], dim=0), val_k_label + test_k_label, seen_gt, unseen_gt, ks,
                                                searched_threshold=searched_threshold, with_predictions=with_predictions)
