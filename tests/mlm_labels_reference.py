"""Restatements for the masked-LM label tests (CPU, numpy / plain torch): BERT's Bernoulli 80/10/10 sampler of clibd_amd.mlm
(`mask_tokens_bert`), the label compaction, the capacity rule, and the objective with HF-style labels and an attention mask on the oracle.

The sampler has no outside oracle at the bit level (HF's collator draws from torch's generator): this file IS its specification.
  i = b S + s;  T(p) = floor(p 2^32 + 0.5);  u0 = lowbias32(i ^ seed), u1 = lowbias32(u0 + G), u2 = lowbias32(u0 + 2 G) mod 2^32, G = 0x9E3779B9
  eligible iff s >= 1, attention_mask[b, s] != 0 and ids[b, s] not in special_ids;  chosen iff eligible and u0 < T(p)
  a chosen id becomes mask_id if u1 < T(replace[0]); else len(special_ids) + ((u2 (V - len(special_ids))) >> 32) if u1 < T(replace[0]) +
  T(replace[1]); else stays.  labels = the original id where chosen, -100 elsewhere.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlm_reference as MR  # noqa: E402
from mlm_reference import O  # noqa: E402

IGNORE = -100
PAD_ROW = -1
GOLDEN = 0x9E3779B9
_M32 = np.uint64(0xFFFFFFFF)


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def threshold(p):
    return int(math.floor(float(p) * 4294967296.0 + 0.5))


def draws(n, seed):
    """(u0, u1, u2) uint64 [n] of the flat positions 0 .. n - 1"""
    u0 = lowbias32(np.arange(n, dtype=np.uint64) ^ np.uint64(int(seed) & 0xFFFFFFFF))
    return u0, lowbias32(u0 + np.uint64(GOLDEN)), lowbias32(u0 + np.uint64(2 * GOLDEN))


def sample_bert(ids, attention_mask, V, seed, p=0.15, mask_id=0, special_ids=(0, 1, 2), replace=(0.8, 0.1, 0.1)):
    """ids int64 [B, S] (numpy or torch), attention_mask [B, S] or None -> (masked, labels), numpy int64 [B, S]"""
    ids = np.asarray(ids, dtype=np.int64)
    B, S = ids.shape
    flat = ids.reshape(-1)
    eligible = (np.arange(B * S) % S) != 0
    if attention_mask is not None:
        eligible &= np.asarray(attention_mask).reshape(-1) != 0
    for sp in special_ids:
        eligible &= flat != sp
    u0, u1, u2 = draws(B * S, seed)
    chosen = eligible & (u0 < np.uint64(threshold(p)))
    t_mask, t_rand = threshold(replace[0]), threshold(replace[0]) + threshold(replace[1])
    ns = len(special_ids)
    rand = (ns + ((u2 * np.uint64(V - ns)) >> np.uint64(32))).astype(np.int64)
    out = np.where(u1 < np.uint64(t_mask), np.int64(mask_id), np.where(u1 < np.uint64(t_rand), rand, flat))
    masked = np.where(chosen, out, flat)
    labels = np.where(chosen, flat, np.int64(IGNORE))
    return masked.reshape(B, S), labels.reshape(B, S)


def compact(labels, r_cap):
    """labels int64 [...] -> (rows int32 [r_cap], targets int64 [r_cap], n, overflow): the labelled flat positions ascending, cut at r_cap,
    then padding"""
    flat = np.asarray(labels, dtype=np.int64).reshape(-1)
    idx = np.nonzero(flat != IGNORE)[0]
    n = idx.size
    rows = np.full(r_cap, PAD_ROW, dtype=np.int32)
    targets = np.full(r_cap, IGNORE, dtype=np.int64)
    k = min(n, r_cap)
    rows[:k] = idx[:k]
    targets[:k] = flat[idx[:k]]
    return rows, targets, n, n > r_cap


def capacity(M, p=None):
    full = (M + 63) // 64 * 64
    if p is None:
        return full
    n = math.ceil(M * min(1.0, p + 6.0 * math.sqrt(p * (1.0 - p) / M)))
    return min(full, max(64, (n + 63) // 64 * 64))


# ---- the objective on the oracle ------------------------------------------------------------------------------------------------------------
def labels_loss(om, input_ids, attention_mask, labels):
    """BertForMaskedLM(input_ids, attention_mask, labels).loss on the oracle: its encoder with HF's additive key mask, then the vocabulary
    head of mlm_reference.mlm_loss on the labelled rows.  Returns (loss, hits)."""
    x = om.bert(input_ids, None, attention_mask)
    flat = labels.reshape(-1)
    rows = torch.nonzero(flat != IGNORE).squeeze(1)
    targets = flat[rows]
    xg = x.reshape(-1, x.shape[-1])[rows]
    t, d = om.cls.predictions.transform, om.cls.predictions.decoder
    h = t.LayerNorm(O._rg(O.gelu_erf(O.olinear(xg, t.dense.weight, t.dense.bias))))
    logits = O.olinear(h, d.weight, d.bias)
    loss = F.cross_entropy(logits, targets, reduction="sum") / max(int(rows.numel()), 1)
    return loss, int((logits.argmax(-1) == targets).sum())


# ---- the learning test's recipe: mlm_reference.LEARN's model, batch and optimizer; a ragged mask; one fixed draw of the bert sampler ---------
LEARN_LENGTHS = (33, 33, 20, 33, 9, 33, 27, 2)      # live keys per sequence (S = 33); the rest is padding (<UNK>, mask 0)
LEARN_SEED, LEARN_P = 777, 0.3


def learn_inputs():
    """(ids, attention_mask) int64 [8, 33] of the fixed batch, and the (masked, labels) the bert sampler draws from it at LEARN_SEED"""
    ids, _ = MR.learn_batch()
    ids = ids.clone()
    mask = torch.zeros_like(ids)
    for b, n in enumerate(LEARN_LENGTHS):
        mask[b, :n] = 1
        ids[b, n:] = 2
    masked, labels = sample_bert(ids.numpy(), mask.numpy(), MR.LEARN["config"]["vocab_size"], LEARN_SEED, p=LEARN_P)
    return ids, mask, torch.from_numpy(masked.copy()), torch.from_numpy(labels.copy())


def oracle_learning_curve(steps, shapes):
    """the recipe in the fp32 oracle on the CPU (tied, torch.optim.AdamW): the loss before every step and after the last"""
    L = MR.LEARN
    sd = MR.synth_state(L["seed"], shapes)
    sd["cls.predictions.decoder.weight"], sd["cls.predictions.decoder.bias"] = sd["bert.embeddings.word_embeddings.weight"], sd["cls.predictions.bias"]
    om = MR.oracle_for(L["config"], sd, True).train()
    opt = torch.optim.AdamW(list(om.parameters()), lr=L["lr"], weight_decay=L["weight_decay"])
    _, mask, masked, labels = learn_inputs()
    curve = []
    for _ in range(steps):
        opt.zero_grad()
        loss, _ = labels_loss(om, masked, mask, labels)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    with torch.no_grad():
        curve.append(float(labels_loss(om, masked, mask, labels)[0]))
    return curve


# ---- the golden's cases: a pure function of the case's name, so the generator (tools/make_mlm_labels_golden.py) and the tests agree ----------
A = dict(vocab_size=259, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, max_position_embeddings=136)
D = dict(vocab_size=259, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=136)
CASES = [("A17", A, 17), ("A33", A, 33), ("D133", D, 133)]   # name, config, S; B = 4


def case_inputs(name):
    """(input_ids, attention_mask, labels), int64 [4, S], of a golden case:
      sequence 0  every key live; many labels (the bert sampler at p = 0.3, 80/10/10);
      sequence 1  one live key beyond position 0 (prefix length 2); ONE label, at position 1;
      sequence 2  a prefix of S // 2 live keys; NO label;
      sequence 3  every key live but a hole over positions S // 3 .. S // 3 + 2; many labels, one more at position 0 and one at a
                  position inside the hole (a padded query row that is labelled)."""
    ci = [c[0] for c in CASES].index(name)
    cfg, S = CASES[ci][1], CASES[ci][2]
    V, B = cfg["vocab_size"], 4
    g = torch.Generator().manual_seed(4100 + ci)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, 2:] = 0
    mask[2, S // 2:] = 0
    mask[3, S // 3:S // 3 + 3] = 0
    ids[1, 2:] = 2
    ids[2, S // 2:] = 2
    masked, labels = sample_bert(ids.numpy(), None, V, 9000 + ci, p=0.3)
    masked, labels = torch.from_numpy(masked.copy()), torch.from_numpy(labels.copy())
    masked[1], labels[1] = ids[1], IGNORE
    masked[2], labels[2] = ids[2], IGNORE
    labels[1, 1] = ids[1, 1]
    masked[1, 1] = 0
    labels[3, 0] = 1                       # position 0 labelled with a special id: allowed in caller-made labels
    labels[3, S // 3 + 1] = ids[3, S // 3 + 1]
    return masked, mask, labels
