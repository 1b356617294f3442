"""Seen/unseen classification by a similarity threshold (the reference's scripts/method_nn.py) on the device.

A query is searched against the SEEN keys (image -> image, source A) and the UNSEEN keys (image -> DNA, source B); prediction j comes
from A if A's j-th similarity exceeds a threshold and from B otherwise.  The threshold maximises the harmonic mean of the seen and the
unseen split's top-1 species accuracy over a grid of 1 000 values; micro / macro / per-class accuracy of the merged predictions are
reported at it.

Where the reference rebuilds a Python list of merged label dicts per threshold and per split, clibd_threshold_sweep_hits counts the
hits of every threshold in one launch and clibd_threshold_merge + clibd_topk_label_hits score the chosen one.  Only integer counts
return to the host, where the reference's float64 arithmetic is restated exactly.  Two conventions, as in clibd_amd.eval:
the reference's lists (function names and signatures of scripts/method_nn.py) and device tensors (`seen_unseen_from_features`).

Stated divergences: a `k_list` without 1 is a ValueError (the reference: KeyError on micro_acc[1]); rows of unequal length, more than 8
predictions per query, a confidence that is not an fp32 value and `best_threshold=None` are ValueErrors; each loader is embedded once
(the reference embeds the queries twice); no tqdm bar, hydra, wandb or CSV output."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import eval as E
from . import ops
from .eval import LEVELS, LabelCodec

SPECIES = LEVELS.index("species")
_A_KEYS = ("pred_labels_from_search_with_seen_keys", "pred_similarity_from_search_with_seen_keys", "pred_labels_from_search_with_unseen_keys", "gt_label")
_B_KEYS = ("pred_labels_from_a", "pred_confidence_from_a", "pred_labels_from_b", "gt_labels")


def _k_list_of(args, k_list) -> List[int]:
    if k_list is None:
        if args is None:
            raise ValueError("method_nn: pass args (args.inference_and_eval_setting.k_list) or k_list=")
        k_list = args.inference_and_eval_setting.k_list
    return E._check_k_list(list(k_list))


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def harmonic_mean(l):
    """len(l) / (1/l[0] + 1/l[1] + ...), summed left to right; 0 as soon as an element is 0 (scripts/method_nn.py:128-135)"""
    s = 0
    for i in l:
        if i == 0:
            return 0
        s = s + 1 / i
    return len(l) / s


# ================================================================================================================ host finaliser
def harmonic_curve(top1_hits: np.ndarray, split_sizes: Sequence[int]) -> List[float]:
    """top1_hits int [T, n_splits] (species hits at k = 1) -> the harmonic mean of acc = hits * 1.0 / Q per threshold, in float64"""
    sizes = [int(n) for n in split_sizes]
    return [harmonic_mean([int(h) * 1.0 / n for h, n in zip(row, sizes)]) for row in np.asarray(top1_hits).tolist()]


def choose_threshold(top1_hits: np.ndarray, split_sizes: Sequence[int], thresholds: np.ndarray):
    """The reference's arg-max (scripts/method_nn.py:138-164): the FIRST threshold whose harmonic mean is strictly greater than the
    running maximum, which starts at -inf: a plateau keeps its first threshold, an all-zero curve yields thresholds[0]."""
    best, max_score = None, float("-inf")
    for threshold, score in zip(thresholds, harmonic_curve(top1_hits, split_sizes)):
        if score > max_score:
            max_score, best = score, threshold
    return best


def _grid(num_intervals: int, thresholds) -> np.ndarray:
    t = np.linspace(0, 1, num_intervals) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if t.size < 1:
        raise ValueError("method_nn: need at least one threshold")
    return t


# ================================================================================================================ list convention
def _conf_f32(conf) -> np.ndarray:
    c64 = np.asarray(conf, dtype=np.float64)
    if c64.ndim != 2 or c64.shape[0] == 0 or not 1 <= c64.shape[1] <= 8:
        raise ValueError("method_nn: confidences must be [Q, m] with Q >= 1 and 1 <= m <= 8 (rows of one length)")
    c32 = c64.astype(np.float32)
    if not np.array_equal(c32.astype(np.float64), c64, equal_nan=True):
        raise ValueError("method_nn: the kernels compare fp32 confidences (in fp64); a confidence here is not an fp32 value")
    return c32


def _encode_pred(codec: LabelCodec, pred_list, m: int) -> np.ndarray:
    """[{level: [m labels]}] -> int32 [Q * m, L] (row q * m + j: the labels of query q's rank j)"""
    out = np.empty((len(pred_list) * m, len(LEVELS)), dtype=np.int32)
    for l, level in enumerate(LEVELS):
        mp = codec.maps[l]
        col = [mp.setdefault(lab, len(mp)) for p in pred_list for lab in p[level][:m]]
        if len(col) != out.shape[0]:
            raise ValueError("method_nn: every prediction list needs one label per confidence")
        out[:, l] = col
    return out


class _Lists:
    """One or more splits of the list convention on the device: ONE codec over A's labels, B's labels and the queries, the predicted
    labels as two key tables [Q * m, L] and the identity as indices (row q of a search = keys q * m .. q * m + m - 1)."""

    def __init__(self, splits):
        self.codec = LabelCodec()
        confs = [_conf_f32(s[1]) for s in splits]
        self.m = confs[0].shape[1]
        self.sizes = [c.shape[0] for c in confs]
        for (pa, _, pb, gt), c in zip(splits, confs):
            if c.shape[1] != self.m or not (len(pa) == len(pb) == len(gt) == c.shape[0]):
                raise ValueError("method_nn: predictions, confidences and ground truth must agree in length (and in m across splits)")
        ta = np.concatenate([_encode_pred(self.codec, s[0], self.m) for s in splits])
        tb = np.concatenate([_encode_pred(self.codec, s[2], self.m) for s in splits])
        self.gt_ids = [self.codec.encode(s[3]) for s in splits]
        dev = _device()
        Q = sum(self.sizes)
        self.table_a_h, self.table_b_h = ta, tb
        self.table_a, self.table_b = torch.from_numpy(ta).to(dev), torch.from_numpy(tb).to(dev)
        self.q_ids = torch.from_numpy(np.concatenate(self.gt_ids)).to(dev)
        self.conf = torch.from_numpy(np.concatenate(confs)).to(dev)
        self.idx = torch.arange(Q * self.m, dtype=torch.int64, device=dev).reshape(Q, self.m)
        self.segment = torch.from_numpy(np.repeat(np.arange(len(splits), dtype=np.int32), self.sizes)).to(dev)

    def sweep(self, thresholds: np.ndarray, ks: Sequence[int]) -> np.ndarray:
        t = torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float64)).to(self.conf.device)
        return ops.threshold_sweep_hits(self.conf, self.idx, self.idx, self.table_a, self.table_b, self.q_ids, t, ks, segment=self.segment,
                                        nseg=len(self.sizes)).cpu().numpy()

    def merge(self, threshold):
        n = self.table_a.shape[0]
        return ops.threshold_merge(self.conf, self.idx, self.idx, n, n, float(threshold))

    def decode(self, merged: torch.Tensor) -> List[dict]:
        return self.codec.decode_rows(np.concatenate([self.table_a_h, self.table_b_h]), merged.cpu().numpy())


def _split_tuple(split: dict):
    for names in (_A_KEYS, _B_KEYS):
        if all(n in split for n in names):
            return tuple(split[n] for n in names)
    raise KeyError(f"method_nn: a split needs the keys {_A_KEYS} or {_B_KEYS}")


def _need_threshold(threshold):
    if threshold is None:
        raise ValueError("method_nn: a threshold is needed (search_threshold_with_harmonic_mean finds one)")
    return threshold


def decide_prediction_with_threshold(args, pred_labels_from_image_classifier, confidence_score_or_similarity, pred_labels_from_search, threshold):
    """The merged prediction lists at one threshold (scripts/method_nn.py:66-91): rank j from the first source where its j-th confidence
    is > threshold, else from the second.  Selected by clibd_threshold_merge; only the label lists are decoded on the host."""
    if len(pred_labels_from_image_classifier) == 0:
        return []
    lists = _Lists([(pred_labels_from_image_classifier, confidence_score_or_similarity, pred_labels_from_search,
                     [{lv: None for lv in LEVELS}] * len(pred_labels_from_image_classifier))])
    merged, _ = lists.merge(_need_threshold(threshold))
    return lists.decode(merged)


def make_final_pred(args, pred_labels_from_search_with_seen_keys, similarity_from_search_with_seen_keys, pred_labels_from_search_with_unseen_keys,
                    gt_labels, threshold):
    return decide_prediction_with_threshold(args, pred_labels_from_search_with_seen_keys, similarity_from_search_with_seen_keys,
                                            pred_labels_from_search_with_unseen_keys, threshold), gt_labels


def sweep_top1_hits(all_split_data, thresholds: np.ndarray) -> np.ndarray:
    """int [T, n_splits]: per threshold and split, the queries whose species equals the merged top-1 prediction.  ONE sweep launch for
    every split (one segment each)."""
    lists = _Lists([_split_tuple(s) for s in all_split_data])
    return lists.sweep(thresholds, [1])[:, :, 0, SPECIES]


def search_threshold_with_harmonic_mean(args, all_split_data, num_intervals=1000, thresholds=None, k_list=None):
    """The threshold of `thresholds` (default np.linspace(0, 1, num_intervals)) that maximises the harmonic mean over the splits of the
    merged predictions' top-1 species accuracy (scripts/method_nn.py:138-164)."""
    if 1 not in _k_list_of(args, k_list):
        raise ValueError("method_nn: the threshold search reads the top-1 accuracy, k_list must contain 1")
    grid = _grid(num_intervals, thresholds)
    hits = sweep_top1_hits(all_split_data, grid)
    return choose_threshold(hits, [len(_split_tuple(s)[3]) for s in all_split_data], grid)


def get_final_pred_and_acc(args, pred_labels_from_search_with_seen_keys, similarity_from_search_with_seen_keys,
                           pred_labels_from_search_with_unseen_keys, gt_labels, best_threshold=None, k_list=None):
    """The merged predictions of one split at `best_threshold` and their micro / macro / per-class accuracy (scripts/method_nn.py:94-109)."""
    ks = _k_list_of(args, k_list)
    lists = _Lists([(pred_labels_from_search_with_seen_keys, similarity_from_search_with_seen_keys, pred_labels_from_search_with_unseen_keys, gt_labels)])
    merged, _ = lists.merge(_need_threshold(best_threshold))
    kk = sorted({min(k, lists.m) for k in ks})              # pred[level][:k] with k beyond the list is the whole list
    off = lists.codec.class_offset()
    _, lh, ch, cc = ops.topk_label_hits(merged, torch.cat([lists.table_a, lists.table_b]), lists.q_ids, off, kk)
    micro, macro, per_class = E._split_accuracy(lh.cpu().numpy()[0], ch.cpu().numpy()[0], cc.cpu().numpy()[0], lists.gt_ids[0], lists.codec, off, ks,
                                                [kk.index(min(k, lists.m)) for k in ks])
    return {"final_pred_labels": lists.decode(merged), "gt_labels": gt_labels, "best_threshold": best_threshold,
            "micro_acc": micro, "macro_acc": macro, "per_class_acc": per_class}


# ============================================================================================================== device convention
def _prepared(keys, dev):
    if isinstance(keys, ops.KeyBank):
        return keys, keys.keys.shape[0]
    k = E._as_device(keys, dev)
    Nk, D = k.shape
    eligible = D % 64 == 0 and D <= ops.KeyBank.MAX_D and 4096 <= Nk < ops.KeyBank.MAX_KEYS
    return (E.prepare_key_bank(k) if eligible else k), Nk


def seen_unseen_from_sources(conf, idx_a, idx_b, labels_a, labels_b, seen_gt, unseen_gt, ks, searched_threshold, grid, with_predictions=True):
    """What follows the two sources of a seen/unseen method, shared by method_nn (A: the seen-key search) and method_linear (A: the
    classifier): conf fp32 [Q, m] and idx_a int64 [Q, m] index `labels_a`, idx_b int64 [Q, m] indexes `labels_b`, the Q queries are the
    seen split followed by the unseen one.  The threshold sweep over `grid` (skipped when `searched_threshold` is given), the merge at
    the chosen threshold and ONE clibd_topk_label_hits launch on the merged indices; returns the reference's two output dicts."""
    dev = conf.device
    Qs, Qu = len(seen_gt), len(unseen_gt)
    Nka, Nkb = len(labels_a), len(labels_b)
    codec = LabelCodec()                                   # one codec: ids agree across the two key sets and the queries
    ids_a, ids_b = codec.encode(labels_a), codec.encode(labels_b)
    s_ids, u_ids = codec.encode(seen_gt), codec.encode(unseen_gt)
    table_a, table_b = torch.from_numpy(ids_a).to(dev), torch.from_numpy(ids_b).to(dev)
    q_ids = torch.from_numpy(np.concatenate([s_ids, u_ids])).to(dev)
    segment = torch.from_numpy(np.repeat(np.array([0, 1], dtype=np.int32), [Qs, Qu])).to(dev)
    if searched_threshold is None:
        hits = ops.threshold_sweep_hits(conf, idx_a, idx_b, table_a, table_b, q_ids, torch.from_numpy(np.ascontiguousarray(grid)).to(dev), [1],
                                        segment=segment, nseg=2).cpu().numpy()[:, :, 0, SPECIES]
        best = choose_threshold(hits, [Qs, Qu], grid)
    else:
        best = searched_threshold
    merged, _ = ops.threshold_merge(conf, idx_a, idx_b, Nka, Nkb, float(best))
    off = codec.class_offset()
    _, lh, ch, cc = ops.topk_label_hits(merged, torch.cat([table_a, table_b]), q_ids, off, ks, segment=segment, nseg=2)
    lh, ch, cc = lh.cpu().numpy(), ch.cpu().numpy(), cc.cpu().numpy()
    rows = list(range(len(ks)))
    merged_h = merged.cpu().numpy()
    if with_predictions:
        preds = codec.decode_rows(np.concatenate([ids_a, ids_b]), merged_h)
        preds = (preds[:Qs], preds[Qs:])
    else:
        preds = (merged_h[:Qs], merged_h[Qs:])
    out = []
    for s, (ids, gt) in enumerate(((s_ids, seen_gt), (u_ids, unseen_gt))):
        micro, macro, per_class = E._split_accuracy(lh[s], ch[s], cc[s], ids, codec, off, ks, rows)
        out.append({"final_pred_labels": preds[s], "gt_labels": gt, "best_threshold": best, "micro_acc": micro, "macro_acc": macro,
                    "per_class_acc": per_class})
    return out[0], out[1]


def seen_unseen_from_features(seen_query, unseen_query, seen_keys, seen_keys_label, unseen_keys, unseen_keys_label, seen_gt, unseen_gt, k_list,
                              searched_threshold=None, thresholds=None, with_predictions=True, num_intervals=1000, max_k=5):
    """method_1_inference_and_eval_for_seen_and_unseen from features (device tensors, numpy arrays, or prepared `KeyBank`s for the keys):
    both searches with the seen and unseen queries concatenated (each key set prepared once), the threshold sweep (skipped when
    `searched_threshold` is given), the merge at the chosen threshold and ONE clibd_topk_label_hits launch on the merged indices.
    Returns the reference's (seen_output_dict, unseen_output_dict); with_predictions=False stores the merged int64 index arrays
    [Q, m] (indices into seen_keys_label + unseen_keys_label) instead of label lists.  m = max(max_k, max(k_list)): the reference
    searches with max_k = 5."""
    ks = E._check_k_list(list(k_list))
    if searched_threshold is None and 1 not in ks:
        raise ValueError("method_nn: the threshold search reads the top-1 accuracy, k_list must contain 1")
    m = max(int(max_k), ks[-1])
    if m > 8:
        raise ValueError("method_nn: at most 8 predictions per query")
    tensors = [x for x in (seen_query, unseen_query, seen_keys, unseen_keys) if torch.is_tensor(x) and x.is_cuda]
    dev = tensors[0].device if tensors else _device()
    Qs, Qu = len(seen_gt), len(unseen_gt)
    queries = torch.cat([E._as_device(seen_query, dev), E._as_device(unseen_query, dev)], dim=0)
    if queries.shape[0] != Qs + Qu or Qs == 0 or Qu == 0:
        raise ValueError("method_nn: one ground-truth label per query, and both splits non-empty")
    bank_a, Nka = _prepared(seen_keys, dev)
    bank_b, Nkb = _prepared(unseen_keys, dev)
    if Nka != len(seen_keys_label) or Nkb != len(unseen_keys_label) or min(Nka, Nkb) < m:
        raise ValueError(f"method_nn: one label per key, and at least {m} keys per key set")
    conf, idx_a = E.topk_search(queries, bank_a, m, cache=False)
    _, idx_b = E.topk_search(queries, bank_b, m, cache=False)
    grid = _grid(num_intervals, thresholds) if searched_threshold is None else None
    return seen_unseen_from_sources(conf, idx_a, idx_b, seen_keys_label, unseen_keys_label, seen_gt, unseen_gt, ks, searched_threshold, grid,
                                    with_predictions)


def inference_with_original_image_encoder_and_dna_encoder(original_model, seen_query_dataloader, unseen_query_dataloader, key_dataloaders, device,
                                                          key_type="dna"):
    """scripts/method_nn.py:22-63 with the reference's return convention (label lists and numpy similarity arrays): the image features of
    both query loaders searched against the concatenated image or DNA features of the key loaders, max_k = 5."""
    if key_type not in ("image", "dna"):
        raise ValueError("key_type must be either 'image' or 'dna'.")
    _, seen_q, _, _, seen_gt = E.get_feature_and_label(seen_query_dataloader, original_model, device, as_numpy=False)
    _, unseen_q, _, _, unseen_gt = E.get_feature_and_label(unseen_query_dataloader, original_model, device, as_numpy=False)
    feats, labels = [], []
    for dl in key_dataloaders:
        _, img, dna, _, lab = E.get_feature_and_label(dl, original_model, device, as_numpy=False)
        feats.append(img if key_type == "image" else dna)
        labels = labels + lab
    bank, _ = _prepared(torch.cat(feats, dim=0), torch.device(device))
    seen_pred, seen_sim = E.make_prediction(seen_q, bank, labels, with_similarity=True, max_k=5)
    unseen_pred, unseen_sim = E.make_prediction(unseen_q, bank, labels, with_similarity=True, max_k=5)
    return seen_pred, seen_sim, seen_gt, unseen_pred, unseen_sim, unseen_gt


def method_1_inference_and_eval_for_seen_and_unseen(args, original_model, seen_query_dataloader, unseen_query_dataloader, seen_keys_dataloader,
                                                    val_unseen_keys_dataloader, test_unseen_keys_dataloader, device, searched_threshold=None,
                                                    k_list=None, with_predictions=True):
    """scripts/method_nn.py:177-246.  Every loader is embedded ONCE and stays on the device: image features of the queries and the
    seen keys, DNA features of the val + test unseen keys (concatenated), then `seen_unseen_from_features`."""
    ks = _k_list_of(args, k_list)
    _, seen_q, _, _, seen_gt = E.get_feature_and_label(seen_query_dataloader, original_model, device, as_numpy=False)
    _, unseen_q, _, _, unseen_gt = E.get_feature_and_label(unseen_query_dataloader, original_model, device, as_numpy=False)
    _, seen_k, _, _, seen_k_label = E.get_feature_and_label(seen_keys_dataloader, original_model, device, as_numpy=False)
    _, _, val_k, _, val_k_label = E.get_feature_and_label(val_unseen_keys_dataloader, original_model, device, as_numpy=False)
    _, _, test_k, _, test_k_label = E.get_feature_and_label(test_unseen_keys_dataloader, original_model, device, as_numpy=False)
    if seen_q is None or unseen_q is None or seen_k is None or val_k is None or test_k is None:
        raise ValueError("method_nn: the model needs an image and a DNA encoder")
    return seen_unseen_from_features(seen_q, unseen_q, seen_k, seen_k_label, torch.cat([val_k, test_k], dim=0), val_k_label + test_k_label,
                                     seen_gt, unseen_gt, ks, searched_threshold=searched_threshold, with_predictions=with_predictions)


# ===================================================================================================================== reporting
def print_acc_for_google_doc(seen_output_dict, unseen_output_dict, K_LIST=None):
    """One row per (micro | macro, k): the seen accuracies per level, the unseen ones, then their harmonic means, rounded to 4 digits."""
    ks = [1, 3, 5] if K_LIST is None else K_LIST
    for kind in ("micro_acc", "macro_acc"):
        for k in ks:
            vals = [d[kind][k][level] for d in (seen_output_dict, unseen_output_dict) for level in LEVELS]
            vals += [harmonic_mean([seen_output_dict[kind][k][level], unseen_output_dict[kind][k][level]]) for level in LEVELS]
            print("".join(" " + str(round(v, 4)) for v in vals))


def check_for_acc_about_correct_predict_seen_or_unseen(final_pred_list, species_list):
    """For k = 1, 3, 5: the fraction of queries with a species of `species_list` among their first k merged predictions
    (scripts/method_nn.py:271-285).  Counted by clibd_topk_label_hits: a one-level key table whose label is 1 where the predicted
    species is in the list, every query labelled 1.  Prints the reference's lines and returns {k: fraction}."""
    Q = len(final_pred_list)
    if Q == 0:
        raise ValueError("method_nn: no predictions")
    lens = {len(r["species"]) for r in final_pred_list}
    if len(lens) != 1 or not 1 <= min(lens) <= 8:
        raise ValueError("method_nn: every prediction list must have the same length, 1 to 8")
    m = lens.pop()
    wanted = set(species_list)
    table = np.array([[1 if s in wanted else 0] for r in final_pred_list for s in r["species"]], dtype=np.int32)
    dev = _device()
    kk = sorted({min(k, m) for k in (1, 3, 5)})
    idx = torch.arange(Q * m, dtype=torch.int64, device=dev).reshape(Q, m)
    _, lh, _, _ = ops.topk_label_hits(idx, torch.from_numpy(table).to(dev), torch.ones((Q, 1), dtype=torch.int32, device=dev), [0, 2], kk)
    lh = lh.cpu().numpy()[0, :, 0]
    out = {}
    for k in (1, 3, 5):
        out[k] = int(lh[kk.index(min(k, m))]) * 1.0 / Q
        print(f"for k = {k}: {out[k]}")
    return out
