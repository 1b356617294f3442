"""Eval-side counterparts on the device ("next" rows SURVEY §8f-1/2): k-mer tokenisation of raw barcodes, the embedding loop
`get_feature_and_label` (reference bioscanclip/epoch/inference_epoch.py:43-111) and the top-k retrieval of `make_prediction`
(reference bioscanclip/util/util.py:521-553: sklearn L2-normalise -> faiss.IndexFlatIP -> search(query, max_k) -> label lookup)."""
from __future__ import annotations

import weakref
from typing import List, Sequence

import numpy as np
import torch

from . import augment, ops

LEVELS = ["order", "family", "genus", "species"]


def tokenize_barcodes(sequences: Sequence[str], device, max_len: int = 660, k: int = 5) -> torch.Tensor:
    """[0] + 132 5-mer ids per barcode (truncate / 'N'-pad to 660 nt), as `get_sequence_pipeline` produces."""
    buf = b"".join(s[:max_len].ljust(max_len, "N").encode("ascii", "replace") for s in sequences)
    seq = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).reshape(len(sequences), max_len).copy()).to(device)
    return ops.kmer_tokenize(seq, k)


def convert_label_dict_to_list_of_dict(label_batch: dict) -> List[dict]:
    """inference_epoch.py:8-20: {level: [labels of the batch]} -> [{level: label} per sample]"""
    return [{"order": o, "family": f, "genus": g, "species": s_}
            for o, f, g, s_ in zip(label_batch["order"], label_batch["family"], label_batch["genus"], label_batch["species"])]


def get_feature_and_label(dataloader, model, device, for_open_clip=False, multi_gpu=False, as_numpy=True):
    """The reference's embedding loop (inference_epoch.py:43-111) without its per-batch `.cpu().tolist()` round trips:
    every batch runs the towers under no_grad, the second `F.normalize` of the reference (:87-92) is the L2-norm kernel, and
    the embeddings stay on the device until ONE copy at the end.

    Batches are the reference's 7-tuples (processid, image, dna, input_ids, token_type_ids, attention_mask, label dict); `image` may be
    a packed batch of decoded pixels with eval records (clibd_amd.augment.collate_encoded(..., train=False));
    `dna` may be a tensor of token ids or a list of raw barcode strings (tokenised by the 5-mer kernel; the remote
    BarcodeBERT tokenizer of the newer checkpoints is out of scope, SURVEY §8a-a5').
    Returns (file_name_list, image_features, dna_features, text_features, label_list) like the reference — features as
    float32 numpy arrays [N, D] (as_numpy=True; the reference builds float64 arrays of the same fp32 values) or as device
    tensors (as_numpy=False, e.g. to feed `make_prediction` without leaving the GPU); None for an absent tower."""
    if for_open_clip:
        raise NotImplementedError("open_clip towers are out of scope (DESIGN §8)")
    dev = torch.device(device)
    feats = ([], [], [])
    label_list, file_name_list = [], []
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in dataloader:
                processid_batch, image_input_batch, dna_input_batch, input_ids, token_type_ids, attention_mask, label_batch = batch
                language_input = None
                if getattr(model, "language_encoder", None) is not None:
                    language_input = {"input_ids": input_ids.to(dev), "token_type_ids": token_type_ids.to(dev),
                                      "attention_mask": attention_mask.to(dev)}
                if torch.is_tensor(dna_input_batch):
                    dna_input_batch = dna_input_batch.to(dev)
                elif getattr(model, "dna_encoder", None) is not None:
                    dna_input_batch = tokenize_barcodes(list(dna_input_batch), dev)
                image_in = None
                if getattr(model, "image_encoder", None) is not None:   # packed decoded pixels: the eval transform on the device
                    image_in = augment.apply(image_input_batch, dev) if augment.is_packed(image_input_batch) else image_input_batch.to(dev)
                outs = model(image_in, dna_input_batch, language_input)[:3]
                for store, out in zip(feats, outs):
                    if out is not None:
                        store.append(ops.l2norm_fwd(out.detach().to(torch.float32).contiguous())[0])
                label_list.extend(convert_label_dict_to_list_of_dict(label_batch))
                file_name_list.extend(list(processid_batch))
        if hasattr(model, "join_streams"):
            model.join_streams()
    finally:
        model.train(was_training)
    out = []
    for store in feats:
        if not store:
            out.append(None)
        else:
            t = torch.cat(store, dim=0)
            out.append(t.cpu().numpy() if as_numpy else t)
    return file_name_list, out[0], out[1], out[2], label_list


def prepare_key_bank(keys_feature: torch.Tensor) -> "ops.KeyBank":
    """L2-normalise a key set and prepare it ONCE for the pre-filtered search (what the reference's faiss.IndexFlatIP(dim) +
    index.add(keys) does once per key set, util/util.py:521-526)."""
    kf, _ = ops.l2norm_fwd(keys_feature.detach().to(torch.float32).contiguous())
    return ops.KeyBank(kf)


# One prepared bank per key TENSOR: `make_prediction` is called with the same keys for every query set of an evaluation
# (inference_epoch.py / util.py:521-553 build ONE faiss index per key set), and a bank costs a normalisation, a bf16 image of the
# keys (630 MB at 410 k x 768) and a conversion kernel.  The key is the tensor's storage, shape, strides and version counter, so an
# in-place update of the keys invalidates the entry; only the most recent bank is kept.
_bank_cache: dict = {}


def clear_key_bank_cache() -> None:
    """Drop the cached bank (normalised fp32 keys + their bf16 image: ~1.9 GB at 410 k x 768), e.g. before training resumes after an evaluation."""
    _bank_cache.clear()


def _cached_key_bank(keys_feature: torch.Tensor) -> "ops.KeyBank":
    # the entry must not outlive the caller's tensor (it would pin ~1.9 GB of device memory until the next call) and a tensor
    # whose version counter cannot be read (created under torch.inference_mode()) is simply not cached
    try:
        version = keys_feature._version
    except RuntimeError:
        return prepare_key_bank(keys_feature)
    key = (keys_feature.data_ptr(), tuple(keys_feature.shape), tuple(keys_feature.stride()), keys_feature.dtype, version, str(keys_feature.device))
    hit = _bank_cache.get("entry")
    if hit is not None and hit[0] == key and hit[1]() is keys_feature:
        return hit[2]
    bank = prepare_key_bank(keys_feature)
    _bank_cache["entry"] = (key, weakref.ref(keys_feature), bank)
    weakref.finalize(keys_feature, _drop_entry_of, key)    # the bank goes when the caller's tensor does
    return bank


def _drop_entry_of(key) -> None:
    hit = _bank_cache.get("entry")
    if hit is not None and hit[0] == key:
        _bank_cache.clear()


def topk_search(query_feature: torch.Tensor, keys_feature, max_k: int = 5, exact: bool = False, cache: bool = True):
    """(similarities, indices) of IndexFlatIP.search on L2-normalised features.  `keys_feature`: a tensor, or a bank from
    `prepare_key_bank` (re-used across query batches).  Large banks take the pre-filtered search (bf16 approximate scores, exact
    fp32 re-score of every key inside the rigorous error band: indices and similarities identical to the exact kernel's); queries
    it flags — candidate lists full inside the band, e.g. many duplicate keys — are re-run through the exact kernel.  exact=True
    forces the exact kernel for everything.  cache=False: the prepared bank of a key TENSOR is not kept (a temporary device copy of host keys
    could never hit and would only pin memory)."""
    q, _ = ops.l2norm_fwd(query_feature.detach().to(torch.float32).contiguous())
    bank = keys_feature if isinstance(keys_feature, ops.KeyBank) else None
    if bank is None:
        Nk, D = keys_feature.shape
        if exact or D % 64 != 0 or D > ops.KeyBank.MAX_D or not (4096 <= Nk < ops.KeyBank.MAX_KEYS):
            kf, _ = ops.l2norm_fwd(keys_feature.detach().to(torch.float32).contiguous())
            return ops.topk_ip(q, kf, max_k)
        bank = _cached_key_bank(keys_feature) if cache else prepare_key_bank(keys_feature)
    if exact:
        return ops.topk_ip(q, bank.keys, max_k)
    sim, idx, ovf = ops.topk_ip_fast(q, bank, max_k)
    bad = torch.nonzero(ovf).flatten()          # (host sync: the eval path hands numpy arrays back anyway)
    if bad.numel():
        s2, i2 = ops.topk_ip(q[bad].contiguous(), bank.keys, max_k)
        sim[bad], idx[bad] = s2, i2
    return sim, idx


def make_prediction(query_feature, keys_feature, keys_label: List[dict], with_similarity=False, with_indices=False, max_k=5, device=None):
    """Same return convention as the reference `make_prediction`: a list of {level: [k predicted labels]} per query,
    optionally followed by the similarity and index arrays (numpy, like faiss).
    `keys_feature`: a device tensor (its prepared bank is cached per tensor and re-used by later calls), a `KeyBank` from
    `prepare_key_bank` (evaluating several query sets against one key set: prepare it once, as the reference builds one faiss index),
    or host data (numpy / CPU tensor: copied and prepared on every call — there is no cheap way to know a host array is unchanged)."""
    dev = device or (query_feature.device if torch.is_tensor(query_feature) else torch.device("cuda"))
    qf = torch.as_tensor(np.asarray(query_feature) if not torch.is_tensor(query_feature) else query_feature).to(dev)
    kf = keys_feature if isinstance(keys_feature, ops.KeyBank) else \
        torch.as_tensor(np.asarray(keys_feature) if not torch.is_tensor(keys_feature) else keys_feature).to(dev)
    # only a tensor the CALLER holds on the device can hit the cache again; host keys (numpy, the reference's convention) become a fresh device copy per call
    on_device = torch.is_tensor(keys_feature) and keys_feature.device == kf.device if torch.is_tensor(kf) else False
    sim, idx = topk_search(qf, kf, max_k, cache=on_device)
    idx_h, sim_h = idx.cpu().numpy(), sim.cpu().numpy()
    pred_list = [{level: [keys_label[i][level] for i in row] for level in LEVELS} for row in idx_h]
    out = [pred_list]
    if with_similarity:
        out.append(sim_h)
    if with_indices:
        out.append(idx_h)
    return out[0] if len(out) == 1 else out


# ================================================================================================================================
# The eval phase (reference scripts/train_cl.py:73-86,124-143 and bioscanclip/util/util.py:379-395,555-742): every query type x key
# type x {seen, unseen} search scored on the device (clibd_topk_label_hits); only integer counts come back to the host, where the
# reference's float64 arithmetic is restated exactly.
QUERY_FEATURE_TYPES = ["encoded_image_feature", "encoded_dna_feature", "encoded_language_feature", "averaged_feature", "concatenated_feature"]
KEY_FEATURE_TYPES = QUERY_FEATURE_TYPES + ["all_key_features"]


class LabelCodec:
    """Per level, one dict mapping every label seen so far (keys first, then queries) to a dense int32 id.  Labels must be hashable
    and equal by `==` (as `gt_label in pred_labels` compares them); NaN labels are unsupported."""

    def __init__(self, levels: Sequence[str] = LEVELS):
        self.levels = list(levels)
        self.maps = [dict() for _ in self.levels]

    def encode(self, label_list: Sequence[dict]) -> np.ndarray:
        """int32 [N, L] ids of a list of {level: label}; labels not seen before get the next free id of their level."""
        out = np.empty((len(label_list), len(self.levels)), dtype=np.int32)
        for l, level in enumerate(self.levels):
            m = self.maps[l]
            out[:, l] = [m.setdefault(d[level], len(m)) for d in label_list]
        return out

    def labels(self, l: int) -> list:
        """The labels of level l in id order."""
        return list(self.maps[l])

    def _table(self, l: int) -> np.ndarray:
        t = np.empty(len(self.maps[l]), dtype=object)    # (filled one by one: tuple labels must stay single objects)
        for i, lab in enumerate(self.maps[l]):
            t[i] = lab
        return t

    def decode(self, ids: np.ndarray) -> List[dict]:
        """int [N, L] ids -> [{level: label}] (the inverse of `encode`)."""
        ids = np.asarray(ids)
        per_level = [self._table(l)[ids[:, l]].tolist() for l in range(len(self.levels))]
        return [dict(zip(self.levels, row)) for row in zip(*per_level)]

    def decode_rows(self, key_ids: np.ndarray, idx: np.ndarray) -> List[dict]:
        """[{level: [labels of the keys idx[q, :]]}] per query, the reference's make_prediction lists; key_ids int [Nk, L]."""
        per_level = [self._table(l)[key_ids[idx, l]].tolist() for l in range(len(self.levels))]
        return [dict(zip(self.levels, row)) for row in zip(*per_level)]

    def class_offset(self) -> List[int]:
        """[0, n_0, n_0 + n_1, ...]: the per-level class axes flattened into one (clibd_topk_label_hits' class_offset)."""
        off = [0]
        for m in self.maps:
            off.append(off[-1] + len(m))
        return off


# Key-side label ids, next to the key-bank cache: an eval phase searches the same key labels with every query type.  Label LISTS are
# matched by identity (the entry holds the list, so its id cannot be reused); a list mutated in place is not detected.
_label_cache: dict = {}
_LABEL_CACHE_ENTRIES = 4


def _cached_key_label_ids(keys_label: list, device):
    key = (id(keys_label), str(device))
    hit = _label_cache.get(key)
    if hit is not None and hit[0] is keys_label and hit[1] == len(keys_label):
        return hit[2], hit[3]
    codec = LabelCodec()
    ids = torch.from_numpy(codec.encode(keys_label)).to(device)
    if len(_label_cache) >= _LABEL_CACHE_ENTRIES:
        _label_cache.pop(next(iter(_label_cache)))
    _label_cache[key] = (keys_label, len(keys_label), codec, ids)
    return codec, ids


def clear_eval_caches() -> None:
    """Drop the cached key bank and the cached key-label ids."""
    clear_key_bank_cache()
    _label_cache.clear()


def _check_k_list(k_list) -> List[int]:
    ks = [int(k) for k in k_list]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 1 or ks[-1] > 8:
        raise ValueError(f"k_list must be strictly ascending with 1 <= k <= 8, got {list(k_list)}")
    return ks


def _split_accuracy(level_hits: np.ndarray, class_hits: np.ndarray, class_count: np.ndarray, query_ids: np.ndarray, codec: LabelCodec,
                    offset: Sequence[int], k_list: Sequence[int], k_rows: Sequence[int]):
    """Integer counts of one query split -> (micro, macro, per_class) in the reference's float64 arithmetic (util.py:379-395,555-599):
      micro[k][level] = hits * 1.0 / Q;
      per_class[k][level][label] = hits_c * 1.0 / count_c over the split's ground-truth labels in order of first appearance;
      macro[k][level] = a sequential left-to-right float64 sum of those, divided by their number (np.cumsum adds in order; np.sum
      would add pairwise and differ in the last bits).
    level_hits [n_k', L], class_hits [n_k', C], class_count [C]; k_rows[i]: the row of k_list[i]."""
    Q = query_ids.shape[0]
    micro, macro, per_class = {}, {}, {}
    order, names = [], []
    for l in range(len(codec.levels)):
        u, first = np.unique(query_ids[:, l], return_index=True)
        ids = u[np.argsort(first, kind="stable")]
        order.append(offset[l] + ids.astype(np.int64))
        lab = codec.labels(l)
        names.append([lab[i] for i in ids.tolist()])
    for k, j in zip(k_list, k_rows):
        micro[k], macro[k], per_class[k] = {}, {}, {}
        for l, level in enumerate(codec.levels):
            micro[k][level] = int(level_hits[j, l]) * 1.0 / Q
            vals = class_hits[j, order[l]].astype(np.float64) / class_count[order[l]].astype(np.float64)
            macro[k][level] = float(np.cumsum(vals)[-1]) / len(vals)
            per_class[k][level] = dict(zip(names[l], vals.tolist()))
    return micro, macro, per_class


def _as_device(x, device) -> torch.Tensor:
    if torch.is_tensor(x):
        return x.detach().to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)


def _score_prediction_lists(pred_list, gt_list, k_list):
    """The reference's list-of-dicts convention on the hits kernel: the predicted labels become a small key table [Q * m, L] and
    the indices are the identity (row q of the search = keys q*m .. q*m + m - 1)."""
    ks = _check_k_list([1, 3, 5] if k_list is None else k_list)
    Q = len(pred_list)
    if Q == 0 or len(gt_list) != Q:
        raise ValueError("top-k accuracy: need as many ground-truth labels as predictions, and at least one")
    lens = {len(p[level]) for p in pred_list for level in LEVELS}
    if len(lens) != 1 or 0 in lens:
        raise ValueError("top-k accuracy: every prediction list must have the same, non-zero length")
    m = min(lens.pop(), ks[-1])
    kk = sorted({min(k, m) for k in ks})           # pred[level][:k] with k beyond the list is the whole list
    codec = LabelCodec()
    keys = np.empty((Q * m, len(LEVELS)), dtype=np.int32)
    for l, level in enumerate(LEVELS):
        mp = codec.maps[l]
        keys[:, l] = [mp.setdefault(lab, len(mp)) for p in pred_list for lab in p[level][:m]]
    gt = codec.encode(gt_list)
    dev = torch.device("cuda", torch.cuda.current_device())
    idx = torch.from_numpy(np.arange(Q * m, dtype=np.int64).reshape(Q, m)).to(dev)
    off = codec.class_offset()
    _, lh, ch, cc = ops.topk_label_hits(idx, torch.from_numpy(keys).to(dev), torch.from_numpy(gt).to(dev), off, kk)
    lh, ch, cc = lh.cpu().numpy()[0], ch.cpu().numpy()[0], cc.cpu().numpy()[0]
    return _split_accuracy(lh, ch, cc, gt, codec, off, ks, [kk.index(min(k, m)) for k in ks])


def top_k_micro_accuracy(pred_list, gt_list, k_list=None):
    """{k: {level: fraction of queries whose label is among the first k predicted}} (reference util.py:379-395), counted on the GPU."""
    return _score_prediction_lists(pred_list, gt_list, k_list)[0]


def top_k_macro_accuracy(pred_list, gt_list, k_list=None):
    """({k: {level: mean per-class accuracy}}, {k: {level: {label: accuracy}}}) (reference util.py:555-599), counted on the GPU."""
    _, macro, per_class = _score_prediction_lists(pred_list, gt_list, k_list)
    return macro, per_class


def get_features_and_label(dataloader, model, device, for_key_set=False, for_open_clip=False, as_numpy=True):
    """The reference's per-split dictionary (util.py:702-742): the three embeddings of `get_feature_and_label`, their average and
    concatenation (clibd_eval_pair_features; fp32, unnormalised as the reference stores them) and, for a key set with all three
    towers, `all_key_features` = image | dna | text keys with the labels repeated three times.  as_numpy=False keeps every
    feature a device tensor."""
    file_name_list, img, dna, text, label_list = get_feature_and_label(dataloader, model, device, for_open_clip=for_open_clip, as_numpy=False)
    averaged = concatenated = all_keys = all_keys_label = None
    if img is not None and dna is not None:
        averaged, concatenated = ops.eval_pair_features(img, dna)
    if for_key_set and img is not None and dna is not None and text is not None:
        all_keys = torch.cat([img, dna, text], dim=0)
        all_keys_label = label_list + label_list + label_list
    conv = (lambda t: None if t is None else t.cpu().numpy()) if as_numpy else (lambda t: t)
    return {
        "file_name_list": file_name_list,
        "encoded_dna_feature": conv(dna),
        "encoded_image_feature": conv(img),
        "encoded_language_feature": conv(text),
        "averaged_feature": conv(averaged),
        "concatenated_feature": conv(concatenated),
        "label_list": label_list,
        "all_key_features": conv(all_keys),
        "all_key_features_label": all_keys_label,
    }


def _print_acc_table(acc_dict, k_list) -> None:
    head = ["query -> key", "acc", "k"] + [f"{s} {lv}" for s in ("seen", "unseen") for lv in LEVELS]
    print(" | ".join(head))
    for qt, per_key in acc_dict.items():
        for kt, per_split in per_key.items():
            if not per_split:
                continue
            for kind in ("micro_acc", "macro_acc"):
                for k in k_list:
                    vals = [f"{per_split[s][kind][k][lv]:.4f}" for s in ("seen", "unseen") for lv in LEVELS]
                    print(" | ".join([f"{qt} -> {kt}", kind, str(k)] + vals))


def inference_and_print_result(keys_dict, seen_dict, unseen_dict, args=None, small_species_list=None, k_list=None, with_predictions=True):
    """The reference's inference_and_print_result (util.py:601-700): the same loop order over query type x key type, the same
    skip rules (absent or None features, a feature width that differs from the keys'; `all_key_features` searched with its own
    labels) and the same return triple (acc_dict, per_class_acc, pred_dict).

    Per key type the keys are prepared once (one bank for the pre-filtered search at >= 4 096 keys) and re-used by every query
    type; the seen and unseen queries go through ONE search and ONE clibd_topk_label_hits launch (segment 0 / 1).  Only integer
    counts (and, for pred_dict, the index arrays) come back to the host.  with_predictions=False stores the int64 index arrays
    [Q, max_k] in pred_dict instead of the reference's per-query label lists.  Prints a plain table (the reference's CSV output and
    `args` header are not reproduced).  Stated divergence: fewer keys than max(k_list) is a ValueError (faiss returns -1 there)."""
    k_list = _check_k_list([1, 3, 5] if k_list is None else k_list)
    max_k = k_list[-1]
    seen_gt, unseen_gt = seen_dict["label_list"], unseen_dict["label_list"]
    keys_label = keys_dict["label_list"]
    if "processed_id_list" in seen_dict and "processed_id_list" in unseen_dict:
        pred_dict = {"seen_id": seen_dict["processed_id_list"], "seen_gt_label": seen_gt,
                     "unseen_id": unseen_dict["processed_id_list"], "unseen_gt_label": unseen_gt}
    else:
        pred_dict = {"seen_id": seen_dict.get("file_name_list", []), "seen_gt_label": seen_gt,
                     "unseen_id": unseen_dict.get("file_name_list", []), "unseen_gt_label": unseen_gt}
    tensors = [v for d in (keys_dict, seen_dict, unseen_dict) for v in d.values() if torch.is_tensor(v) and v.is_cuda]
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    Qs, Qu = len(seen_gt), len(unseen_gt)
    segment = torch.from_numpy(np.repeat(np.array([0, 1], dtype=np.int32), [Qs, Qu])).to(dev)
    prepared = {}     # key type -> KeyBank (pre-filtered search) or device keys (exact search), shared by every query type
    encoded = {}      # id(codec) -> (device ids of seen | unseen, host ids of seen, host ids of unseen)
    acc_dict, per_class_acc = {}, {}
    for qt in QUERY_FEATURE_TYPES:
        if qt not in seen_dict:
            continue
        acc_dict[qt], per_class_acc[qt], pred_dict[qt] = {}, {}, {}
        queries = None
        for kt in KEY_FEATURE_TYPES:
            if kt not in keys_dict:
                continue
            acc_dict[qt][kt], per_class_acc[qt][kt], pred_dict[qt][kt] = {}, {}, {}
            sf, uf, kf = seen_dict[qt], unseen_dict[qt], keys_dict[kt]
            if kf is None:
                continue
            if kt == "all_key_features":
                keys_label = keys_dict["all_key_features_label"]   # (and kept for the key types after it, as in the reference)
            if sf is None or uf is None or kf.shape[-1] != sf.shape[-1] or kf.shape[-1] != uf.shape[-1]:
                continue
            Nk, D = kf.shape
            if Nk < max_k:
                raise ValueError(f"{kt}: {Nk} keys cannot fill a top-{max_k} search")
            if kt not in prepared:
                keys = _as_device(kf, dev)
                eligible = D % 64 == 0 and D <= ops.KeyBank.MAX_D and 4096 <= Nk < ops.KeyBank.MAX_KEYS
                prepared[kt] = prepare_key_bank(keys) if eligible else keys
            if queries is None:
                queries = torch.cat([_as_device(sf, dev), _as_device(uf, dev)], dim=0)
            codec, key_ids = _cached_key_label_ids(keys_label, dev)
            if id(codec) not in encoded:
                s_ids, u_ids = codec.encode(seen_gt), codec.encode(unseen_gt)
                encoded[id(codec)] = (torch.from_numpy(np.concatenate([s_ids, u_ids])).to(dev), s_ids, u_ids)
            q_ids, s_ids, u_ids = encoded[id(codec)]
            _, idx = topk_search(queries, prepared[kt], max_k, cache=False)
            off = codec.class_offset()
            _, lh, ch, cc = ops.topk_label_hits(idx, key_ids, q_ids, off, k_list, segment=segment, nseg=2)
            lh, ch, cc = lh.cpu().numpy(), ch.cpu().numpy(), cc.cpu().numpy()
            rows = list(range(len(k_list)))
            s_micro, s_macro, s_per_class = _split_accuracy(lh[0], ch[0], cc[0], s_ids, codec, off, k_list, rows)
            u_micro, u_macro, u_per_class = _split_accuracy(lh[1], ch[1], cc[1], u_ids, codec, off, k_list, rows)
            idx_h = idx.cpu().numpy()
            if with_predictions:
                key_ids_h = key_ids.cpu().numpy()
                pred_dict[qt][kt] = {"curr_seen_pred_list": codec.decode_rows(key_ids_h, idx_h[:Qs]),
                                     "curr_unseen_pred_list": codec.decode_rows(key_ids_h, idx_h[Qs:])}
            else:
                pred_dict[qt][kt] = {"curr_seen_pred_list": idx_h[:Qs], "curr_unseen_pred_list": idx_h[Qs:]}
            acc_dict[qt][kt]["seen"] = {"micro_acc": s_micro, "macro_acc": s_macro}
            acc_dict[qt][kt]["unseen"] = {"micro_acc": u_micro, "macro_acc": u_macro}
            per_class_acc[qt][kt]["seen"] = s_per_class
            per_class_acc[qt][kt]["unseen"] = u_per_class
    _print_acc_table(acc_dict, k_list)
    return acc_dict, per_class_acc, pred_dict


def eval_phase(model, device, all_keys_dataloader, seen_val_dataloader, unseen_val_dataloader, k_list, args=None, species_to_drop=None, rank=None,
               for_open_clip=False, with_predictions=True):
    """The reference's eval_phase (scripts/train_cl.py:73-86): key, seen and unseen features, then every search scored.
    Features stay on the device between the two steps.  Returns (acc_dict, pred_dict)."""
    if for_open_clip:
        raise NotImplementedError("open_clip towers are out of scope (DESIGN §8)")
    keys_dict = get_features_and_label(all_keys_dataloader, model, device, for_key_set=True, as_numpy=False)
    seen_dict = get_features_and_label(seen_val_dataloader, model, device, as_numpy=False)
    unseen_dict = get_features_and_label(unseen_val_dataloader, model, device, as_numpy=False)
    acc_dict, _, pred_dict = inference_and_print_result(keys_dict, seen_dict, unseen_dict, args=args, k_list=k_list, with_predictions=with_predictions)
    return acc_dict, pred_dict


def compute_overall_acc(acc_dict) -> float:
    """The checkpoint-selection number of scripts/train_cl.py:124-143: the mean of every accuracy in acc_dict except those at
    k = 3 and k = 5, summed left to right in acc_dict's order."""
    vals = []
    for per_key in acc_dict.values():
        for per_split in per_key.values():
            for per_kind in per_split.values():
                for table in per_kind.values():
                    for k, per_level in table.items():
                        if k == 3 or k == 5:
                            continue
                        vals.extend(per_level.values())
    return sum(vals) / len(vals)
