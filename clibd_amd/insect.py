"""The INSECT / BZSL workflow (the reference's scripts/BZSL/ and bioscanclip/epoch/fine_tuning_epoch.py) on the device: the aligned image
and DNA encoders fine-tuned jointly under two classification heads, the heads scored by top-k, and the per-image embeddings and
per-class mean DNA embeddings ("class prototypes") written as the two CSV tables that the external Bayesian zero-shot code reads.

Two conventions, as in clibd_amd.method_nn and clibd_amd.method_linear: the reference's lists and loaders (its function names and
signatures) and device tensors (`class_mean_embeddings`, `ops.logits_topk`, `ops.class_mean`).

What runs where: the towers with their backward are the model's; each head's product is method_linear.linear_f32 (split-bf16,
fp32-grade), the loss is method_linear.CrossEntropyLoss, the update one FusedAdamW over both classifiers; the top-k of
the logits is clibd_logits_topk, the hits clibd_topk_label_hits on a one-level table, the class means clibd_class_mean_f32
(include/clibd_hip_insect.h).  The two towers of the joint step run one after the other on the current stream.

Stated divergences:
  - `EncoderWithExtraLayer` trains what its tower differentiates — under LoRA the adapters, the projection head and the new layer, with
    the base weights frozen as in the contrastive training; everything under `disable_lora` — where the reference's script sets
    requires_grad on every parameter (the divergence of method_linear); `train_encoder=False` runs the encoder without gradient;
  - the criterion is method_linear.CrossEntropyLoss (nn.CrossEntropyLoss() with its defaults only); a target outside [0, C) sets bit 0
    of `ops.ce_error_word` instead of raising, and no step synchronises with the host;
  - an epoch's loss is accumulated on the device in fp32 and fetched once (the reference: a float64 mean of per-step `.item()`s);
  - `evaluate_epoch` takes at most 8 indices per sample, and equal logits resolve to the lower index (torch.argsort without
    stable=True promises no order there); NaN logits are not supported;
  - `get_unique_species_for_seen` keeps Python's set order as the reference does — an order that changes from process to process with
    str hashing, so a checkpoint's head only means something together with the list it was trained with; `sort=True` gives a
    reproducible order;
  - `label_batch_to_species_idx` looks species up in a dict of first positions (list.index semantics, ValueError for an unknown one);
  - the class means are float32 sums of the float32 rows that `get_features_and_label` returns, in row order, divided in float32 — bit
    for bit np.sum(rows, axis=0) / len(rows) on such rows (the reference's embedding loop passes through Python lists, so its rows are
    float64 copies of the same fp32 values); `class_embeddings` returns a float32 array where the reference builds an object array
    before np.savetxt: the written text is identical;
  - `construct_key_dict` joins device tensors as well as numpy arrays, and a feature that is None in either dict stays None (the
    reference's np.concatenate raises there);
  - the optimizer is clibd_amd.optim.FusedAdamW (torch.optim.AdamW's update on one flat bucket, a parameter reachable from both
    classifiers listed once); `image_last.ckpt` / `dna_last.ckpt` hold CPU tensors; no hydra, wandb, tqdm or config.yaml.

Out of scope: the INSECT dataset reader (scipy.io.loadmat of res101.mat, the HDF5 file) — the functions here take loaders of the
reference's 7-tuple (processid, image, dna, input_ids, token_type_ids, attention_mask, label dict) and a label array;
scripts/BZSL/method_linear_on_INSECT.py, a near copy of what clibd_amd.method_linear provides; fine_tune_vitb_on_insect.py, a bare timm
ViT, which `EncoderWithExtraLayer` accepts as it is; `convert_acc_dict_to_wandb_dict`; the two towers of the joint step on separate
streams (tools/bench_insect.py records the joint step beside the two single steps as the baseline of such a change)."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import eval as E
from . import ops
from .method_linear import CrossEntropyLoss, _cfg, _images, linear_f32  # noqa: F401

F32 = torch.float32
MAX_K = 8   # clibd_logits_topk keeps eight candidates per lane


# ==================================================================================================================== the model
class EncoderWithExtraLayer(nn.Module):
    """bioscanclip/util/util.py:42-54.  `encoder`: any module that returns device fp32 [B, D] features (CLIBDImageEncoder, CLIBDDNAEncoder,
    a bare ViT); it is wrapped, not copied, so a step trains the model it came from.  `new_linear_layer`: an nn.Linear used as a
    parameter holder — its product is clibd_linear_f32_fwd, its backward clibd_linear_f32_bwd.  State-dict keys: encoder.*,
    new_linear_layer.weight, new_linear_layer.bias, as in the reference's image_last.ckpt / dna_last.ckpt."""

    def __init__(self, encoder, new_linear_layer, train_encoder: bool = True):
        super(EncoderWithExtraLayer, self).__init__()
        self.encoder = encoder
        self.new_linear_layer = new_linear_layer
        self.train_encoder = bool(train_encoder)

    def get_feature(self, x):
        return self.encoder(x)

    def forward(self, x):
        if self.train_encoder:
            outputs = self.encoder(x)
        else:
            with torch.no_grad():
                outputs = self.encoder(x)
        return linear_f32(outputs, self.new_linear_layer.weight, self.new_linear_layer.bias)


def build_classifiers(original_model, num_classes: int, output_dim: int, device=None):
    """supervised_fine_tune_bioscan_clip_model_on_insect.py:67-77: (image_classifier, dna_classifier) over `original_model`'s own
    encoders (no copy), each with a new nn.Linear(output_dim, num_classes)."""
    if getattr(original_model, "image_encoder", None) is None or getattr(original_model, "dna_encoder", None) is None:
        raise ValueError("build_classifiers: the model needs an image and a DNA encoder")
    image_classifier = EncoderWithExtraLayer(original_model.image_encoder, nn.Linear(int(output_dim), int(num_classes)))
    dna_classifier = EncoderWithExtraLayer(original_model.dna_encoder, nn.Linear(int(output_dim), int(num_classes)))
    if device is not None:
        image_classifier, dna_classifier = image_classifier.to(device), dna_classifier.to(device)
    return image_classifier, dna_classifier


def combined_parameters(*modules) -> list:
    """list(image_classifier.parameters()) + list(dna_classifier.parameters()) with a parameter reachable twice listed once"""
    seen, out = set(), []
    for m in modules:
        for p in m.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                out.append(p)
    return out


# ================================================================================================================= host helpers
def get_unique_species_for_seen(dataloader, sort: bool = False):
    """util.py:305-314: the species of a loader, each once, in Python's set order (see the module docstring); sort=True: sorted"""
    all_species = []
    for batch in dataloader:
        all_species = all_species + list(batch[-1]["species"])
    unique_species = list(set(all_species))
    if sort:
        unique_species.sort()
    return unique_species


def species_index(unique_species_for_seen) -> dict:
    """{species: its first position in the list}: list.index as one lookup"""
    if isinstance(unique_species_for_seen, dict):
        return unique_species_for_seen
    index = {}
    for i, species in enumerate(unique_species_for_seen):
        index.setdefault(species, i)
    return index


def label_batch_to_species_idx(label_batch, unique_species_for_seen):
    """fine_tuning_epoch.py:6-9: int64 [B], unique_species_for_seen.index(species) per sample (a list, or its `species_index`)"""
    index = species_index(unique_species_for_seen)
    out = []
    for species in label_batch["species"]:
        if species not in index:
            raise ValueError(f"{species!r} is not in list")
        out.append(index[species])
    return torch.tensor(out, dtype=torch.int64)


def _input_of(batch, modality: str, dev):
    if modality == "image":
        return _images(batch[1], dev)
    if modality == "dna":
        dna = batch[2]
        return dna.to(dev) if torch.is_tensor(dna) else E.tokenize_barcodes(list(dna), dev)
    raise ValueError(f"modality must be 'image' or 'dna', got {modality!r}")


# ================================================================================================================ training loops
def fine_tuning_epoch(args, model, insect_train_dataloader, optimizer, criterion, unique_species_for_seen, epoch, device, modality="image",
                      scheduler=None, step_losses: Optional[list] = None):
    """fine_tuning_epoch.py:11-37, and with `scheduler` scripts/BZSL/fine_tune_bioscan_clip_image_on_insect.py:63-87: one pass over the
    loader on one modality.  No host synchronisation inside a step; `step_losses` (a list) receives every step's device loss.
    Returns the epoch's mean loss (one host fetch)."""
    dev = torch.device(device)
    index = species_index(unique_species_for_seen)
    running = torch.zeros((), dtype=F32, device=dev)
    n = 0
    for batch in insect_train_dataloader:
        target = label_batch_to_species_idx(batch[6], index).to(dev)
        optimizer.zero_grad()
        output = model(_input_of(batch, modality, dev))
        loss = criterion(output, target)
        loss.backward()
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        running += loss.detach()
        if step_losses is not None:
            step_losses.append(loss.detach())
        n += 1
    return float(running.item()) / max(n, 1)          # the one host fetch of the epoch


def fine_tuning_epoch_image_and_dna(args, image_classifier, dna_classifier, insect_train_dataloader, optimizer, criterion, unique_species_for_seen,
                                    epoch, device, step_losses: Optional[list] = None):
    """fine_tuning_epoch.py:77-103: one step is criterion(image_out, t) + criterion(dna_out, t), one backward through both towers and
    one optimizer step over both classifiers.  The towers run one after the other on the current stream; nothing in a step
    synchronises with the host.  Returns the epoch's mean summed loss (one host fetch)."""
    image_classifier.train()
    dna_classifier.train()
    dev = torch.device(device)
    index = species_index(unique_species_for_seen)
    running = torch.zeros((), dtype=F32, device=dev)
    n = 0
    for batch in insect_train_dataloader:
        target = label_batch_to_species_idx(batch[6], index).to(dev)
        optimizer.zero_grad()
        image_output = image_classifier(_input_of(batch, "image", dev))
        dna_output = dna_classifier(_input_of(batch, "dna", dev))
        loss = criterion(image_output, target) + criterion(dna_output, target)
        loss.backward()
        optimizer.step()
        running += loss.detach()
        if step_losses is not None:
            step_losses.append(loss.detach())
        n += 1
    return float(running.item()) / max(n, 1)


def predict_topk(model, dataloader, device, unique_species_for_seen, k: int, modality="image"):
    """(idx int64 [N, k] on the device, target int64 [N] on the host): clibd_logits_topk of the model's logits over a loader"""
    dev = torch.device(device)
    index = species_index(unique_species_for_seen)
    idx_all, targets = [], []
    with torch.no_grad():
        for batch in dataloader:
            targets.append(label_batch_to_species_idx(batch[6], index))
            output = model(_input_of(batch, modality, dev))
            idx_all.append(ops.logits_topk(output, min(int(k), output.shape[1]))[1])
    return torch.cat(idx_all, dim=0), torch.cat(targets)


def evaluate_epoch(model, dataloader, device, unique_species_for_seen, k_values=None, modality="image"):
    """fine_tuning_epoch.py:39-75: {"top{k}_accuracy": the fraction of samples whose class is among the k largest LOGITS} as numpy float64.
    The class indices come from clibd_logits_topk (the reference's torch.argsort(output, descending=True)[:, :max(k)]), the hits are
    counted by clibd_topk_label_hits on a one-level table (class index -> itself); hits / N is np.mean of the reference's boolean
    array.  Leaves the model in eval mode, as the reference does."""
    if k_values is None:
        k_values = [1, 3, 5]
    ks = sorted({int(k) for k in k_values})
    if not ks or ks[0] < 1 or ks[-1] > MAX_K:
        raise ValueError(f"evaluate_epoch: k_values must lie in 1..{MAX_K}")
    model.eval()
    dev = torch.device(device)
    idx, target = predict_topk(model, dataloader, dev, unique_species_for_seen, ks[-1], modality)
    N, m = idx.shape
    n_classes = max(len(species_index(unique_species_for_seen)), int(target.max()) + 1, m)
    table = torch.arange(n_classes, dtype=torch.int32, device=dev).reshape(-1, 1)
    kk = sorted({min(k, m) for k in ks})
    _, lh, _, _ = ops.topk_label_hits(idx, table, target.to(torch.int32).reshape(-1, 1).to(dev), [0, n_classes], kk)
    lh = lh.cpu().numpy()[0, :, 0]
    return {f"top{k}_accuracy": np.float64(int(lh[kk.index(min(int(k), m))])) / N for k in k_values}


# ============================================================================================================== class prototypes
def class_mean_embeddings(features: torch.Tensor, labels, num_classes: Optional[int] = None, transposed: bool = False, check: bool = True):
    """The device form of the prototypes: features fp32 [N, D] on the device, labels [N] (a device or host integer tensor or array) in
    [0, C).  Returns (mean fp32 [C, D] — [D, C] with transposed=True —, count int32 [C]), both on the device: mean[c] is the float32 sum
    of class c's rows in ascending row order divided by their number in float32; a class without rows is a zero row with count 0.
    num_classes=None: max(labels) + 1 (a host fetch).  check=True reads the error word back (a host fetch) and raises ValueError for a
    label outside [0, C); check=False skips such rows silently, without a synchronisation."""
    if not torch.is_tensor(features) or not features.is_cuda:
        raise ValueError("class_mean_embeddings: expected a device tensor (clibd_amd has no CPU compute path)")
    dev = features.device
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    if lab.dim() != 1 or lab.is_floating_point() or lab.dtype == torch.bool:
        raise ValueError("class_mean_embeddings: labels must be a 1-D integer array")
    if num_classes is None:
        num_classes = int(lab.max().item()) + 1 if lab.numel() else 0
    lab = lab.to(device=dev, dtype=torch.int32).contiguous()
    x = features.detach().to(F32)
    if x.dim() != 2 or x.stride(1) != 1:
        x = x.reshape(x.shape[0], -1).contiguous()
    mean, count, error = ops.class_mean(x, lab, int(num_classes), transposed=transposed)
    if check and int(error.item()) & 1:
        raise ValueError(f"class_mean_embeddings: a label outside [0, {int(num_classes)})")
    if x.shape[0] >= 1 << 24 and int(count.max().item()) >= 1 << 24:
        raise ValueError("class_mean_embeddings: a class with 2^24 rows or more (its size is not exact in float32)")
    return mean, count


def class_embeddings(dna_feature, labels) -> np.ndarray:
    """extract_feature_for_insect_dataset.py:79-92 (= supervised_fine_tune_bioscan_clip_model_on_insect.py:157-171): the mean float32 DNA
    embedding of every class of `labels`, classes in np.unique order, as float32 [D, C] (squeezed like the reference's table).
    dna_feature: [N, D] numpy or a device tensor; labels: the N class labels of the rows (any integers)."""
    labels = np.asarray(labels).reshape(-1)
    all_label, dense = np.unique(labels, return_inverse=True)
    dev = dna_feature.device if torch.is_tensor(dna_feature) and dna_feature.is_cuda else torch.device("cuda", torch.cuda.current_device())
    feats = E._as_device(dna_feature, dev)
    if feats.dim() != 2 or feats.shape[0] != labels.shape[0]:
        raise ValueError("class_embeddings: one label per row of dna_feature [N, D]")
    mean, _ = class_mean_embeddings(feats, dense.astype(np.int32), len(all_label), transposed=True)
    return mean.cpu().numpy().squeeze()


def save_bzsl_embeddings(dna_path, image_path, dict_for_feature, labels):
    """The two tables of the BZSL code (extract_feature_for_insect_dataset.py:94-102): `dna_path` gets the prototypes [D, C],
    `image_path` the image features as float32 [D, N], both by np.savetxt(..., delimiter=",").  dict_for_feature: what
    `get_features_and_label` returns (numpy arrays or device tensors).  Returns (class_embed, image_feature) as written."""
    class_embed = class_embeddings(dict_for_feature["encoded_dna_feature"], labels)
    np.savetxt(dna_path, class_embed, delimiter=",")
    image_feature = dict_for_feature["encoded_image_feature"]
    if torch.is_tensor(image_feature):
        image_feature = image_feature.detach().cpu().numpy()
    image_feature = np.asarray(image_feature).astype(np.float32).T
    np.savetxt(image_path, image_feature, delimiter=",")
    return class_embed, image_feature


# ========================================================================================== scripts/BZSL/train_cl_on_insect_dataset.py
def construct_key_dict(list_of_dict):
    """train_cl_on_insect_dataset.py:39-56: the union of several splits' dictionaries as one key set — lists are joined, arrays (numpy or
    device tensors) concatenated along the rows, `all_key_features` and its labels are None."""
    key_dict = {}
    for curr_dict in list_of_dict:
        for name in curr_dict.keys():
            if name == "all_key_features" or name == "all_key_features_label":
                key_dict[name] = None
                continue
            value = curr_dict[name]
            if name not in key_dict.keys():
                key_dict[name] = value
            elif isinstance(value, list):
                key_dict[name] = key_dict[name] + value
            elif value is None or key_dict[name] is None:
                key_dict[name] = None
            elif torch.is_tensor(value):
                key_dict[name] = torch.cat((key_dict[name], value), dim=0)
            else:
                key_dict[name] = np.concatenate((key_dict[name], value), axis=0)
    return key_dict


def eval_phase(model, device, insect_train_dataloader_for_key, insect_val_dataloader, insect_test_seen_dataloader, insect_test_unseen_dataloader,
               k_list, species_to_drop=None, with_predictions=True):
    """train_cl_on_insect_dataset.py:58-75: the keys are the union of all four INSECT loaders, the queries test-seen and test-unseen.
    Every loader is embedded once and its features stay on the device between the two steps.  Returns (acc_dict, pred_dict)."""
    dicts = [E.get_features_and_label(loader, model, device, as_numpy=False)
             for loader in (insect_train_dataloader_for_key, insect_val_dataloader, insect_test_seen_dataloader, insect_test_unseen_dataloader)]
    keys_dict = construct_key_dict(dicts)
    acc_dict, _, pred_dict = E.inference_and_print_result(keys_dict, dicts[2], dicts[3], small_species_list=None, k_list=k_list,
                                                          with_predictions=with_predictions)
    return acc_dict, pred_dict


def overall_acc(acc_dict):
    """train_cl_on_insect_dataset.py:150-153: the mean of the seen and the unseen split's image -> image micro top-1 species accuracy
    (the splits are named "seen" / "unseen" by inference_and_print_result, "seen_val" / "unseen_val" in older dictionaries)"""
    per_split = acc_dict["encoded_image_feature"]["encoded_image_feature"]
    seen = per_split["seen_val"] if "seen_val" in per_split else per_split["seen"]
    unseen = per_split["unseen_val"] if "unseen_val" in per_split else per_split["unseen"]
    return (seen["micro_acc"][1]["species"] + unseen["micro_acc"][1]["species"]) / 2


# =================================================================================================================== the driver
def _save_state(module, path):
    torch.save({k: v.detach().cpu().clone() for k, v in module.state_dict().items()}, path)


def supervised_fine_tune(args, original_model, trainval_loader, test_seen_loader, all_loader, labels, device, out_dir=None, lr: float = 0.001,
                         unique_species_for_seen=None):
    """The epoch loop of supervised_fine_tune_bioscan_clip_model_on_insect.py:56-182.  The two classifiers wrap `original_model`'s own
    encoders; FusedAdamW(lr=1e-3) over both; `args.model_config.fine_tuning_set.epochs` epochs of `fine_tuning_epoch_image_and_dna`;
    every `args.model_config.evaluation_period` epochs both heads are scored on `test_seen_loader`, and — with args.save_ckpt —
    `<out_dir>/image_last.ckpt` and `dna_last.ckpt` are written, `all_loader` is embedded by the fine-tuned encoders and the two CSV
    tables are exported for `labels` (the class of every row of `all_loader`, the script's res101 `labels`).
    Returns {"epoch_losses", "evaluation": [(epoch, image dict, dna dict)], "image_classifier", "dna_classifier",
    "unique_species_for_seen", "image_last_ckpt_path", "dna_last_ckpt_path", "dna_embed_path", "image_embed_path"}."""
    from .optim import FusedAdamW

    dev = torch.device(device)
    mc = args.model_config
    get = (lambda node, name, default=None: node.get(name, default) if isinstance(node, dict) else getattr(node, name, default))
    epochs = int(_cfg(args, "epochs"))
    period = int(get(mc, "evaluation_period", 1))
    output_dim = int(get(mc, "output_dim"))
    save_ckpt = bool(getattr(args, "save_ckpt", False))
    if unique_species_for_seen is None:
        unique_species_for_seen = get_unique_species_for_seen(trainval_loader)
    original_model = original_model.to(dev)
    image_classifier, dna_classifier = build_classifiers(original_model, len(unique_species_for_seen), output_dim, dev)
    criterion = CrossEntropyLoss()
    optimizer = FusedAdamW(combined_parameters(image_classifier, dna_classifier), lr=lr)
    out = {"epoch_losses": [], "evaluation": [], "image_classifier": image_classifier, "dna_classifier": dna_classifier,
           "unique_species_for_seen": unique_species_for_seen, "image_last_ckpt_path": None, "dna_last_ckpt_path": None,
           "dna_embed_path": None, "image_embed_path": None}
    if save_ckpt:
        if out_dir is None:
            raise ValueError("supervised_fine_tune: args.save_ckpt needs out_dir")
        os.makedirs(out_dir, exist_ok=True)
        out["image_last_ckpt_path"] = os.path.join(out_dir, "image_last.ckpt")
        out["dna_last_ckpt_path"] = os.path.join(out_dir, "dna_last.ckpt")
        out["dna_embed_path"] = os.path.join(out_dir, "dna_embedding_from_bioscan_clip.csv")
        out["image_embed_path"] = os.path.join(out_dir, "image_embedding_from_bioscan_clip.csv")
    for epoch in range(epochs):
        epoch_loss = fine_tuning_epoch_image_and_dna(args, image_classifier, dna_classifier, trainval_loader, optimizer, criterion,
                                                     unique_species_for_seen, epoch, dev)
        out["epoch_losses"].append(epoch_loss)
        if epoch % period == 0:
            print("Eval:")
            image_result = evaluate_epoch(image_classifier, test_seen_loader, dev, unique_species_for_seen, modality="image")
            dna_result = evaluate_epoch(dna_classifier, test_seen_loader, dev, unique_species_for_seen, modality="dna")
            print("Image Evaluation Result:", image_result)
            print("DNA Evaluation Result:", dna_result)
            out["evaluation"].append((epoch, image_result, dna_result))
            if save_ckpt:
                _save_state(image_classifier, out["image_last_ckpt_path"])
                _save_state(dna_classifier, out["dna_last_ckpt_path"])
                print(f"Last image ckpt: {out['image_last_ckpt_path']}")
                print(f"Last dna ckpt: {out['dna_last_ckpt_path']}")
                dict_for_feature = E.get_features_and_label(all_loader, original_model, dev, for_key_set=False, as_numpy=False)
                save_bzsl_embeddings(out["dna_embed_path"], out["image_embed_path"], dict_for_feature, labels)
                print(out["image_embed_path"])
    return out
