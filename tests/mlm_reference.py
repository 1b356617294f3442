"""Restatements for the masked-k-mer pre-training tests (CPU, plain torch): the position sampler of clibd_amd.mlm on the oracle's hash, the
vocabulary head of HF BertForMaskedLM(input_ids, labels) on the oracle's rounding points, the cross-entropy yardsticks (fp64 and an fp32
evaluation of the kernel's formula), the seeded weights of the golden models and the sampling of their gradients.

The sampler has no outside oracle (BarcodeBERT's training code is not part of the reference): this file IS its specification.
  position 0 is never chosen;  key(b, s) = (ids[b, s] == unk, lowbias32((b S + s) ^ seed), s) for s >= 1;  the n_mask smallest keys of a
  sequence are chosen;  chosen ids become mask_id;  target = original id, or -100 where that was unk;  rows = b S + s, ascending.
"""
import hashlib
import os
import sys
import zlib

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import clibd_oracle as O  # noqa: E402

IGNORE = -100


def n_mask_for(S, ratio):
    return max(1, int(ratio * (S - 1)))


def sample(ids, seed, n_mask, mask_id=0, unk_id=2):
    """ids int64 [B, S] -> (masked int64 [B, S], rows int32 [B n_mask], targets int64 [B n_mask], n_valid int32 [1])"""
    B, S = ids.shape
    assert 2 <= S <= 256 and 1 <= n_mask <= S - 1
    flat = torch.arange(B * S, dtype=torch.int64).view(B, S)
    h = O._lowbias32(flat ^ (int(seed) & 0xFFFFFFFF))
    masked, rows, targets = ids.clone(), [], []
    for b in range(B):
        keys = sorted((int(ids[b, s] == unk_id), int(h[b, s]), s) for s in range(1, S))
        for s in sorted(k[2] for k in keys[:n_mask]):
            rows.append(b * S + s)
            targets.append(IGNORE if int(ids[b, s]) == unk_id else int(ids[b, s]))
            masked[b, s] = mask_id
    targets = torch.tensor(targets, dtype=torch.int64)
    return masked, torch.tensor(rows, dtype=torch.int32), targets, torch.tensor([int((targets != IGNORE).sum())], dtype=torch.int32)


# ---- the objective on the oracle ------------------------------------------------------------------------------------------------------
def tie(om):
    """HF's tie_word_embeddings=True on an oracle BertForMaskedLM: the decoder's weight IS the word table, its bias IS predictions.bias"""
    p = om.cls.predictions
    p.decoder.weight = om.bert.embeddings.word_embeddings.weight
    p.decoder.bias = p.bias
    return om


def mlm_loss(om, masked_ids, rows, targets):
    """BertForMaskedLM(masked_ids, labels).loss with labels = -100 off `rows`: the oracle's encoder, then the vocabulary head restated on the
    masked rows only (transform dense, erf GELU, LayerNorm, decoder; the rounding points are olinear's under O.precision("bf16")).
    Returns (loss, hits): the mean over the targets that are not -100 (0 when there are none) and the number of rows whose arg max is
    their target."""
    x = om.bert(masked_ids)
    xg = x.reshape(-1, x.shape[-1])[rows.long()]
    t, d = om.cls.predictions.transform, om.cls.predictions.decoder
    h = t.LayerNorm(O._rg(O.gelu_erf(O.olinear(xg, t.dense.weight, t.dense.bias))))
    logits = O.olinear(h, d.weight, d.bias)
    n = max(int((targets != IGNORE).sum()), 1)
    loss = F.cross_entropy(logits, targets, ignore_index=IGNORE, reduction="sum") / n
    hits = int(((logits.argmax(-1) == targets) & (targets != IGNORE)).sum())
    return loss, hits


def named_grads(om, loss):
    """{HF key: gradient} over the oracle's parameters; a tied parameter under both of its names, an unused one as zeros"""
    ps = dict(om.named_parameters(remove_duplicate=False))
    uniq = list({id(p): p for p in ps.values()}.values())
    gs = dict(zip(map(id, uniq), torch.autograd.grad(loss, uniq, allow_unused=True)))
    return {n: (torch.zeros_like(p) if gs[id(p)] is None else gs[id(p)]).detach() for n, p in ps.items()}


# ---- seeded weights: a pure function of (seed, key, element index), integer arithmetic only, so every machine holds the same bits ----------------
def synth_tensor(seed, key, shape, lo, hi):
    n = 1
    for d in shape:
        n *= d
    base = (zlib.crc32(key.encode()) ^ (int(seed) * 0x9E3779B1)) & 0xFFFFFFFF
    u = O._lowbias32(torch.arange(n, dtype=torch.int64) ^ base).double() / 4294967296.0     # [0, 1)
    return (lo + (hi - lo) * u).float().view(shape)


def synth_state(seed, shapes):
    """shapes: {key: shape} of a BertForMaskedLM state dict.  LayerNorm weights around 1, everything else around 0, nothing exactly zero."""
    sd = {}
    for key, shape in shapes.items():
        if "LayerNorm.weight" in key:
            sd[key] = synth_tensor(seed, key, shape, 0.8, 1.2)
        elif key.endswith("bias"):
            sd[key] = synth_tensor(seed, key, shape, -0.05, 0.05)
        else:
            sd[key] = synth_tensor(seed, key, shape, -0.09, 0.09)
    return sd


def state_hash(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


SAMPLE = 512


def sample_index(key, numel):
    """the elements of a gradient the golden keeps: all of a tensor of at most SAMPLE elements, else SAMPLE hashed positions"""
    if numel <= SAMPLE:
        return None
    return O._lowbias32(torch.arange(SAMPLE, dtype=torch.int64) ^ zlib.crc32(key.encode())) % numel


def sampled(key, g):
    idx = sample_index(key, g.numel())
    return g.reshape(-1).clone() if idx is None else g.reshape(-1)[idx].clone()


def oracle_for(cfg, sd, tied):
    om = O.BertForMaskedLM(vocab=cfg["vocab_size"], hidden=cfg["hidden_size"], layers=cfg["num_hidden_layers"], heads=cfg["num_attention_heads"],
                           ff=cfg["intermediate_size"], max_pos=cfg["max_position_embeddings"])
    om.load_state_dict(sd, strict=True)
    return (tie(om) if tied else om).eval()


# ---- cross-entropy yardsticks --------------------------------------------------------------------------------------------------------------
def ce_reference(logits_bf16, V, targets, dtype):
    """The kernel's formula in `dtype` on the bf16 inputs: max, sum of exp(x - max), row loss = log(sum) + max - x_t, loss = sum / n,
    gradient = (exp(x - max) / sum - onehot) / n with n = max(#targets != -100, 1); ignored rows: loss 0, gradient 0.
    Returns (loss, row_loss [R], grad [R, V] in `dtype`, hits)."""
    x = logits_bf16[:, :V].to(dtype)
    valid = targets != IGNORE
    n = max(int(valid.sum()), 1)
    mx = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - mx)
    s = e.sum(dim=1, keepdim=True)
    t = targets.clamp(min=0)
    row = (torch.log(s) + mx).squeeze(1) - x.gather(1, t[:, None]).squeeze(1)
    row = torch.where(valid, row, torch.zeros_like(row))
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    grad = (e / s - onehot) / n
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    cols = torch.arange(V)[None, :].expand_as(x)
    first_max = torch.where(x == mx, cols, torch.full_like(cols, V)).min(dim=1).values     # the lowest index among the maxima
    hits = int(((first_max == targets) & valid).sum())
    return row.sum() / n, row, grad, hits


def bf16_neighbours_ok(got_bf16, ref64, rel_slack):
    """Every entry of got (bf16) that differs from bf16(ref64) is a NEAR TIE: it is the bf16 neighbour on the other side of a rounding
    boundary that ref64 lies within rel_slack * |ref64| of.  Returns (all ok, number of differing entries)."""
    want = ref64.to(torch.bfloat16)
    diff = got_bf16 != want
    if not diff.any():
        return True, 0
    g, w, r = got_bf16[diff].double(), want[diff].double(), ref64[diff]
    mid = (g + w) / 2          # the boundary between two adjacent bf16 values is their midpoint
    ulp = torch.maximum(w.abs(), g.abs()) * 2.0 ** -7
    adjacent = (g - w).abs() <= ulp * 1.0001
    near = (r - mid).abs() <= rel_slack * r.abs()
    return bool((adjacent & near).all()), int(diff.sum())


CE_SHAPES = [(R, V, ld) for R in (1, 63, 130) for V, ld in ((259, 264), (1027, 1032), (4099, 4104), (8192, 8192))]


def ce_case(R, V, ld, poison=1.0e30):
    """(logits bf16 [R, ld], targets int64 [R]): N(0, 4) logits rounded to bf16, the padding columns V .. ld - 1 filled with `poison`;
    every fifth row ignored (R > 1); planted exact ties for the arg max: row 1 holds its maximum twice and targets the lower column (a hit),
    row 2 the same and targets the higher column (no hit), row 3 targets its single maximum (a hit)."""
    g = torch.Generator().manual_seed(1000 * R + V)
    logits = torch.full((R, ld), poison, dtype=torch.float32)
    logits[:, :V] = 2.0 * torch.randn(R, V, generator=g)
    targets = torch.randint(0, V, (R,), generator=g)
    if R > 3:
        top = float(logits[:, :V].max()) + 1.0
        logits[1, 10], logits[1, V - 3], targets[1] = top, top, 10
        logits[2, 7], logits[2, V - 1], targets[2] = top, top, V - 1
        logits[3, V // 2], targets[3] = top, V // 2
        targets[4::5] = IGNORE
    return logits.to(torch.bfloat16), targets


# ---- the learning test's recipe: one fixed batch, one fixed mask, AdamW ----------------------------------------------------------------------------
LEARN = dict(config=dict(vocab_size=259, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
                         max_position_embeddings=136, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0),
             seed=900, B=8, S=33, mask_seed=4242, ratio=0.5, lr=2e-3, weight_decay=0.01)


def learn_batch():
    g = torch.Generator().manual_seed(LEARN["seed"])
    B, S, V = LEARN["B"], LEARN["S"], LEARN["config"]["vocab_size"]
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1)
    return ids, sample(ids, LEARN["mask_seed"], n_mask_for(S, LEARN["ratio"]))


def oracle_learning_curve(steps, shapes):
    """the recipe in the fp32 oracle on the CPU (tied, torch.optim.AdamW): the loss before every step and after the last"""
    sd = synth_state(LEARN["seed"], shapes)
    sd["cls.predictions.decoder.weight"], sd["cls.predictions.decoder.bias"] = sd["bert.embeddings.word_embeddings.weight"], sd["cls.predictions.bias"]
    om = oracle_for(LEARN["config"], sd, True).train()
    opt = torch.optim.AdamW(list(om.parameters()), lr=LEARN["lr"], weight_decay=LEARN["weight_decay"])
    _, (masked, rows, targets, _) = learn_batch()
    curve = []
    for _ in range(steps):
        opt.zero_grad()
        loss, _ = mlm_loss(om, masked, rows, targets)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    with torch.no_grad():
        curve.append(float(mlm_loss(om, masked, rows, targets)[0]))
    return curve
