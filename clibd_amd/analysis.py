"""Embedding analysis on the device: the arithmetic behind the reference's result scripts, after `inference_and_eval.py` has produced
`keys_dict` / `seen_dict` / `unseen_dict`.

  * silhouette per taxonomic level   calculate_silhouette_score (scripts/inference_and_eval.py, scripts/result/distribution_of_similarities.py
                                     :34-38, scripts/result/check_failure_cases.py): sklearn's silhouette_samples once per level
  * nearest key of the same species  get_similarity_for_different_combination_of_modalities (distribution_of_similarities.py:57-164), for
                                     the nine query / key modality pairs, binned on [0, .3, .6, .9, 1.2, 1.5]
  * confusion matrices               scripts/result/create_confusion_matrix.py: sklearn's confusion_matrix of the top-1 prediction per
                                     (split, query, key, level), rows normalised, the "10 largest" and "10 most confused" sub-matrices

Two conventions, as in method_nn: the reference's names and signatures on its dicts and lists, and device-tensor forms
(`silhouette_samples`, `silhouette_by_level`, `nearest_same_species`, `distance_histogram`, `confusion_from_predictions`).  The kernels are
clibd_silhouette_samples, clibd_same_label_nearest and clibd_confusion_counts (include/clibd_hip_analysis.h); what stays on the host is
label coding (eval.LabelCodec), the stable sort that makes every cluster one run, np.histogram on a fetched [Nq] vector and the top-10
selections on a fetched [C, C] matrix.  No figure is opened anywhere: where the reference plots, these functions return the numbers.

Stated divergences from the reference:
  * the printed silhouette mean is the float64 mean of the fp32 samples; the reference's avg_list is a sequential Python `sum` of float32;
  * the samples themselves come from an fp32 Gram product (sklearn upcasts float32 blocks to float64): DESIGN §3.9 has the error model;
  * class order is sorted; the reference's `list(set(...))` is in hash order, which changes between runs;
  * the np.argsort calls of the two top-10 selections are stable here (equal counts / equal entries keep class order);
  * the reference's `distance_for_image_to_language` column holds the DNA -> language distance; that is reproduced under the same name,
    and the image -> language distance is returned under `distance_for_true_image_to_language`;
  * a query species without a key raises KeyError in the list convention (the reference's dict lookup); `nearest_same_species` returns
    +inf and -1 for it;
  * duplicate query file names collapse to the last record at the first one's position (the reference keys a dict by file name);
  * fewer than 2 or more than N - 1 clusters raises ValueError with sklearn's condition;
  * the CSV is written (with the csv module, every record key a column) only when `args` carries `project_root_path`.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .eval import LEVELS, LabelCodec

BINS = [0.0, 0.3, 0.6, 0.9, 1.2, 1.5]
QUERY_AND_KEY_FEATURES = ["encoded_image_feature", "encoded_dna_feature", "encoded_language_feature"]
QUERY_AND_KEY_WE_CARE_ABOUT = [("encoded_image_feature", "encoded_image_feature"), ("encoded_dna_feature", "encoded_dna_feature"),
                               ("encoded_image_feature", "encoded_dna_feature")]
K_STEP = 32        # the silhouette kernel's K-step: a width it does not divide is zero padded (no distance changes)
TRUE_IMAGE_TO_LANGUAGE = "distance_for_true_image_to_language"


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def _dev(x, device=None) -> torch.Tensor:
    """fp32 contiguous device tensor of a tensor or an array"""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if not x.is_cuda:
        x = x.to(device if device is not None else _device())
    return x.to(torch.float32).contiguous()


# ---- planning (host) --------------------------------------------------------------------------------------------------------------------
def plan_clusters(codes) -> tuple:
    """(order int64 [N], seg int32 [C + 1]): the stable permutation that makes every cluster one run, clusters by ascending code, and
    the run offsets.  Codes need not be dense."""
    codes = np.asarray(codes.detach().cpu().numpy() if torch.is_tensor(codes) else codes)
    if codes.ndim != 1:
        raise ValueError("plan_clusters: codes must be 1-D")
    order = np.argsort(codes, kind="stable")
    _, counts = np.unique(codes, return_counts=True)
    seg = np.zeros(len(counts) + 1, dtype=np.int32)
    np.cumsum(counts, out=seg[1:])
    return order.astype(np.int64), seg


def plan_groups(key_codes, num_classes: int) -> tuple:
    """(order int64 [Nk], seg int32 [C + 1]) for keys with dense class codes in [0, C): classes without a key keep an empty run"""
    key_codes = np.asarray(key_codes)
    order = np.argsort(key_codes, kind="stable")
    seg = np.zeros(num_classes + 1, dtype=np.int32)
    np.cumsum(np.bincount(key_codes, minlength=num_classes), out=seg[1:])
    return order.astype(np.int64), seg


def chunk_plan(N: int, col_chunk: int = 0) -> List[tuple]:
    """the column chunks [c0, c1) of the silhouette kernel (0 = its default width of 1024)"""
    cc = 1024 if col_chunk == 0 else int(col_chunk)
    if cc <= 0 or cc % 64 != 0:
        raise ValueError("col_chunk must be 0 or a positive multiple of 64")
    return [(c0, min(c0 + cc, N)) for c0 in range(0, N, cc)]


def pad_width(x: torch.Tensor, multiple: int = K_STEP) -> torch.Tensor:
    D = x.shape[1]
    Dp = -(-D // multiple) * multiple
    if Dp == D:
        return x
    out = torch.zeros((x.shape[0], Dp), dtype=x.dtype, device=x.device)
    out[:, :D] = x
    return out


# ---- silhouette ---------------------------------------------------------------------------------------------------------------------------
def silhouette_samples(features, codes, col_chunk: int = 0) -> torch.Tensor:
    """sklearn's silhouette_samples(features, codes) as a device fp32 [N] tensor in the caller's row order.  features [N, D] (tensor or
    array), codes int [N] (any integers; equal code = same cluster)."""
    if len(features.shape) != 2:
        raise ValueError("silhouette_samples: features must be [N, D]")
    N = features.shape[0]
    order, seg = plan_clusters(codes)
    if len(order) != N:
        raise ValueError("silhouette_samples: one code per row")
    n_labels = len(seg) - 1
    if not 1 < n_labels < N:
        raise ValueError(f"Number of labels is {n_labels}. Valid values are 2 to n_samples - 1 (inclusive)")
    x = _dev(features)
    order_d = torch.from_numpy(order).to(x.device)
    xs = pad_width(x.index_select(0, order_d))
    s_sorted = ops.silhouette_samples(xs, seg, col_chunk)
    out = torch.empty_like(s_sorted)
    out[order_d] = s_sorted
    return out


def silhouette_by_level(features, label_list: Sequence[dict], levels: Sequence[str] = LEVELS, col_chunk: int = 0) -> Dict[str, torch.Tensor]:
    """{level: device fp32 [N] silhouette samples} for a list of {level: label}"""
    ids = LabelCodec(levels).encode(label_list)
    if not torch.is_tensor(features):
        features = np.asarray(features)
    for l in range(len(levels)):         # every level's condition before any device work
        n_labels = len(np.unique(ids[:, l]))
        if not 1 < n_labels < len(ids):
            raise ValueError(f"Number of labels is {n_labels}. Valid values are 2 to n_samples - 1 (inclusive)")
    x = _dev(features)
    return {level: silhouette_samples(x, ids[:, l], col_chunk) for l, level in enumerate(levels)}


def calculate_silhouette_score(args, image_features, labels) -> Dict[str, float]:
    """The reference's calculate_silhouette_score(args, image_features, labels): `labels[1]` is the list of label dicts.  Prints its four
    lines and also returns {level: mean}."""
    per_level = silhouette_by_level(image_features, labels[1])
    out = {}
    for level in LEVELS:
        out[level] = float(per_level[level].cpu().numpy().astype(np.float64).mean())
        print(f"The silhouette score for {level} level is : {out[level]}")
    return out


# ---- nearest key of the same species ------------------------------------------------------------------------------------------------------
class _Groups:
    """keys grouped by species once, shared by every modality pair"""

    def __init__(self, key_labels: Sequence, device):
        self.codec = LabelCodec(["species"])
        key_codes = self.codec.encode([{"species": s} for s in key_labels])[:, 0]
        self.n_classes = len(self.codec.maps[0])
        order, self.seg = plan_groups(key_codes, self.n_classes)
        self.order = torch.from_numpy(order).to(device)
        self.device = device

    def query_classes(self, query_labels: Sequence) -> np.ndarray:
        m = self.codec.maps[0]
        return np.array([m.get(s, -1) for s in query_labels], dtype=np.int32)

    def nearest(self, q: torch.Tensor, k: torch.Tensor, qclass_d: torch.Tensor):
        dist, arg = ops.same_label_nearest(q, k.index_select(0, self.order), self.seg, qclass_d)
        arg = arg.to(torch.int64)
        return dist, torch.where(arg >= 0, self.order[arg.clamp_min(0)], arg)


def nearest_same_species(query_feats, key_feats, query_labels: Sequence, key_labels: Sequence):
    """(dist fp32 [Nq], arg int64 [Nq]) on the device: the Euclidean distance from each query to the nearest key with the query's label
    and that key's row in key_feats (the lowest row on a tie); +inf and -1 where no key carries the label."""
    q = _dev(query_feats)
    k = _dev(key_feats, q.device)
    if len(query_labels) != q.shape[0] or len(key_labels) != k.shape[0]:
        raise ValueError("nearest_same_species: one label per row")
    g = _Groups(key_labels, q.device)
    return g.nearest(q, k, torch.from_numpy(g.query_classes(query_labels)).to(q.device))


def distance_histogram(distances, bins: Sequence[float] = BINS) -> np.ndarray:
    """np.histogram counts of a distance vector on the reference's bins (host arithmetic on the fetched result)"""
    d = distances.detach().cpu().numpy() if torch.is_tensor(distances) else np.asarray(distances)
    return np.histogram(d.astype(np.float64), bins=bins)[0]


def get_similarity_for_different_combination_of_modalities(keys_dict, seen_dict, unseen_dict, args=None) -> List[dict]:
    """The reference's function of this name: per query the distance to the nearest key of its species for the nine modality pairs,
    returned as the list of records behind its DataFrame (its column names; see the module docstring for `distance_for_image_to_language`).
    The CSV is written when `args.project_root_path` exists; the histogram of the figure is `distance_histograms(records)`."""
    key_species = {d["species"] for d in keys_dict["label_list"]}
    for query_dict in (seen_dict, unseen_dict):
        for d in query_dict["label_list"]:
            if d["species"] not in key_species:
                raise KeyError(d["species"])
    device = _device()
    groups = _Groups([d["species"] for d in keys_dict["label_list"]], device)
    keys = {f: _dev(keys_dict[f], device) for f in QUERY_AND_KEY_FEATURES}
    eval_on = getattr(getattr(args, "inference_and_eval_setting", None), "eval_on", None)
    records = []
    for split, query_dict in (("seen", seen_dict), ("unseen", unseen_dict)):
        labels = query_dict["label_list"]
        species = [d["species"] for d in labels]
        qclass = groups.query_classes(species)
        if (qclass < 0).any():
            raise KeyError(species[int(np.nonzero(qclass < 0)[0][0])])
        qclass_d = torch.from_numpy(qclass).to(device)
        dist = {}
        for qf in QUERY_AND_KEY_FEATURES:
            q = _dev(query_dict[qf], device)
            for kf in QUERY_AND_KEY_FEATURES:
                dist[f"{qf}_{kf}"] = groups.nearest(q, keys[kf], qclass_d)[0].cpu().numpy()
        position = {}
        for i, name in enumerate(query_dict["processed_id_list"]):
            position[name] = i
        for name, i in position.items():
            d = {k: float(v[i]) for k, v in dist.items()}
            records.append({
                "file_name": name, "order": labels[i]["order"], "family": labels[i]["family"], "genus": labels[i]["genus"],
                "species": labels[i]["species"],
                "distance_for_image_to_image": d["encoded_image_feature_encoded_image_feature"],
                "distance_for_dna_to_dna": d["encoded_dna_feature_encoded_dna_feature"],
                "distance_for_image_to_dna": d["encoded_image_feature_encoded_dna_feature"],
                "distance_for_dna_to_image": d["encoded_dna_feature_encoded_image_feature"],
                "distance_for_image_to_language": d["encoded_dna_feature_encoded_language_feature"],
                "split": f"{eval_on}_{split}",
                TRUE_IMAGE_TO_LANGUAGE: d["encoded_image_feature_encoded_language_feature"],
            })
    root = getattr(args, "project_root_path", None)
    if root is not None and records:
        folder_path = os.path.join(root, "distribution_of_similarities")
        os.makedirs(folder_path, exist_ok=True)
        with open(os.path.join(folder_path, f"{eval_on}_query_info_with_distance_to_nearest_key_with_same_species.csv"), "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(records[0]))
            w.writeheader()
            w.writerows(records)
        print(f"Saved the query info with distance to nearest key with same species at {folder_path}")
    return records


def distance_histograms(records: Sequence[dict], bins: Sequence[float] = BINS) -> Dict[str, np.ndarray]:
    """the four series of the reference's figure: counts per bin of the image-to-image, DNA-to-DNA, image-to-DNA and (its) image-to-text
    columns"""
    cols = {"Image-to-Image": "distance_for_image_to_image", "DNA-to-DNA": "distance_for_dna_to_dna", "Image-to-DNA": "distance_for_image_to_dna",
            "Image-to-Text": "distance_for_image_to_language"}
    return {name: distance_histogram(np.array([r[c] for r in records]), bins) for name, c in cols.items()}


# ---- confusion ------------------------------------------------------------------------------------------------------------------------------
def _counts(true_code: np.ndarray, pred_code: np.ndarray, num_classes: int, device=None) -> np.ndarray:
    device = device if device is not None else _device()
    t = torch.from_numpy(np.ascontiguousarray(true_code, dtype=np.int32)).to(device)
    p = torch.from_numpy(np.ascontiguousarray(pred_code, dtype=np.int32)).to(device)
    return ops.confusion_counts(t, p, num_classes).cpu().numpy().astype(np.int64)


def confusion_matrix(y_true: Sequence, y_pred: Sequence, labels: Sequence) -> np.ndarray:
    """sklearn.metrics.confusion_matrix(y_true, y_pred, labels=labels): int64 [C, C], rows = true; a sample whose true or predicted label
    is not in `labels` is not counted."""
    if len(y_true) != len(y_pred):
        raise ValueError("confusion_matrix: y_true and y_pred differ in length")
    if len(labels) == 0:
        raise ValueError("'labels' should contains at least one label.")
    m = {c: i for i, c in enumerate(labels)}
    if len(y_true) == 0:
        return np.zeros((len(labels), len(labels)), dtype=np.int64)
    return _counts(np.array([m.get(v, -1) for v in y_true]), np.array([m.get(v, -1) for v in y_pred]), len(labels))


def normalized_confusion(cm: np.ndarray) -> np.ndarray:
    """rows divided by their sums, an empty row all zero (the reference's nan_to_num)"""
    cm = np.asarray(cm)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.nan_to_num(cm.astype("float") / cm.sum(axis=1, keepdims=True))


def _largest_10(cm: np.ndarray, class_labels: Sequence):
    idx = np.argsort(-np.diag(cm), kind="stable")[0:10]
    return normalized_confusion(cm)[np.ix_(idx, idx)], [class_labels[i] for i in idx]


def _most_confused_10(cm: np.ndarray, class_labels: Sequence):
    cmn = normalized_confusion(cm)
    masked = np.copy(cmn)
    np.fill_diagonal(masked, -np.inf)
    pairs = np.dstack(np.unravel_index(np.argsort(-masked.ravel(), kind="stable"), masked.shape))[0]
    unique = set()
    for i, j in pairs:
        unique.update([int(i), int(j)])
        if len(unique) >= 10:
            break
    unique = sorted(unique)[:10]
    return cmn[np.ix_(unique, unique)], [class_labels[i] for i in unique]


def largest_10_classes(y_pred, y_true, class_labels):
    """(sub_matrix, labels) of the reference's plot_confusion_matrix_with_largest_10_classes: the ten classes with the most correct
    predictions, the normalised matrix restricted to them"""
    return _largest_10(confusion_matrix(y_true, y_pred, class_labels), class_labels)


def most_confused_10_classes(y_pred, y_true, class_labels):
    """(sub_matrix, labels) of the reference's plot_confusion_matrix_with_10_most_confused_classes: the classes of the largest
    off-diagonal normalised entries until ten are collected, in class order"""
    return _most_confused_10(confusion_matrix(y_true, y_pred, class_labels), class_labels)


def confusion_from_predictions(pred_dict: dict, keys_label: Optional[Sequence[dict]] = None, pairs=QUERY_AND_KEY_WE_CARE_ABOUT) -> dict:
    """The reference's plot_confusion_matrix(pred_dict) without the figures: result[split][(query, key)][level] = {"labels": the sorted
    classes of the ground truth, "cm": int64 counts, "largest": (sub_matrix, labels), "most_confused": (sub_matrix, labels)}.
    The prediction lists are the reference's per-query {level: [labels]} or, from inference_and_print_result(..., with_predictions=False),
    the int index arrays [Q, max_k] into the keys; the latter needs `keys_label`, the label list of those keys."""
    out = {}
    for split in ("seen", "unseen"):
        gt_list = pred_dict[f"{split}_gt_label"]
        out[split] = {}
        for query, key in pairs:
            pred_list = pred_dict[query][key][f"curr_{split}_pred_list"]
            codec = LabelCodec()
            if isinstance(pred_list, (np.ndarray, torch.Tensor)):
                if keys_label is None:
                    raise ValueError("confusion_from_predictions: index arrays need keys_label")
                idx = pred_list.detach().cpu().numpy() if torch.is_tensor(pred_list) else pred_list
                pred_ids = codec.encode(keys_label)[idx[:, 0]]
            else:
                pred_ids = codec.encode([{lv: p[lv][0] for lv in LEVELS} for p in pred_list])
            gt_ids = codec.encode(gt_list)
            per_level = {}
            for l, level in enumerate(LEVELS):
                classes = sorted({g[level] for g in gt_list})
                table = np.full(len(codec.maps[l]), -1, dtype=np.int32)
                for rank, c in enumerate(classes):
                    table[codec.maps[l][c]] = rank
                cm = _counts(table[gt_ids[:, l]], table[pred_ids[:, l]], len(classes))
                per_level[level] = {"labels": classes, "cm": cm, "largest": _largest_10(cm, classes), "most_confused": _most_confused_10(cm, classes)}
            out[split][(query, key)] = per_level
    return out
