"""Time of the masked-LM pre-training step with HF-style labels (clibd_amd.mlm) beside the fixed-count step, on one MI355X.

    python tools/bench_mlm_labels.py [--batch 256] [--iters 10] [--windows 5] [--out profiles/mlm_labels.log]

BERT-base BarcodeBERT (12 layers x 12 heads of 64, hidden 768, k = 5: vocabulary 1027, S = 133), train mode, tied weights, FusedAdamW.
One process; the four forms ALTERNATE inside every window (a, b, c, d, a, b, ...), device events, medians over the windows:
  a  the fixed-count step: mask_tokens(ratio 0.5) + model(masked, rows, targets, n_valid) + backward + optimizer step — the parent's code;
  b  the HF-style step fed the same rows: mask_tokens + model(input_ids=, labels=, label_capacity = the row count) + backward + step;
  c  pretrain_step(sampler="bert", mlm_probability=0.15), default capacity (six binomial standard deviations over the mean);
  d  c with a ragged attention mask (lengths uniform in S / 2 .. S): the masked attention kernels.
And alone, at the same M = batch x S: the label compaction, the bert sampler, the fixed-count sampler.
Records, not gates.  Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("bench_mlm_labels.py measures on an MI355X: no GPU found")
    from clibd_amd import mlm, ops
    from clibd_amd.build import csrc_hash
    from clibd_amd.model import BertConfigLite, BertForMaskedLM
    from clibd_amd.optim import FusedAdamW

    dev = torch.device("cuda:0")
    V, B, S, ratio, p = 1027, a.batch, 133, 0.5, 0.15
    torch.manual_seed(0)
    model = mlm.BarcodeBERTForPreTraining(BertForMaskedLM(BertConfigLite(vocab_size=V, max_position_embeddings=256))).to(dev).train()
    opt = FusedAdamW(model.parameters(), lr=1e-4)
    model.attach(opt)
    g = torch.Generator().manual_seed(1)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1)
    lengths = torch.randint(S // 2, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None, :] < lengths[:, None]).long()
    ragged_ids = torch.where(mask != 0, ids, torch.full_like(ids, 2)).to(dev)
    ids, mask = ids.to(dev), mask.to(dev)
    masked, rows, targets, n_valid = mlm.mask_tokens(ids, ratio, seed=7)
    count = int(rows.numel())
    assert count % 64 == 0, "the row count must be a multiple of 64 for form b (batch 256: 16 896)"
    labels = torch.full((B * S,), -100, dtype=torch.int64, device=dev)
    labels[rows.long()] = targets
    labels = labels.view(B, S)

    def step_a():
        mlm.pretrain_step(model, ids, opt, ratio, seed=7)

    def step_b():
        m, _, _, _ = mlm.mask_tokens(ids, ratio, seed=7)
        opt.zero_grad()
        loss, _ = model(input_ids=m, labels=labels, label_capacity=count)
        loss.backward()
        opt.step()

    def step_c():
        mlm.pretrain_step(model, ids, opt, sampler="bert", mlm_probability=p)

    def step_d():
        mlm.pretrain_step(model, (ragged_ids, mask), opt, sampler="bert", mlm_probability=p)

    forms = {"a_fixed_count": step_a, "b_labels_same_rows": step_b, "c_bert_sampler": step_c, "d_bert_sampler_ragged_mask": step_d}
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.windows):
        for k, fn in forms.items():
            times[k].append(timed(fn, a.iters))
    _, lab_c = mlm.mask_tokens_bert(ids, None, p, seed=7, vocab_size=V)
    cap = ops.mlm_label_capacity(B * S, p)
    alone = {"compact_default_capacity": lambda: ops.mlm_compact_labels(lab_c, V, cap), "compact_labels_of_b": lambda: ops.mlm_compact_labels(labels, V, count),
             "bert_sampler": lambda: mlm.mask_tokens_bert(ids, None, p, seed=7, vocab_size=V),
             "bert_sampler_masked": lambda: mlm.mask_tokens_bert(ragged_ids, mask, p, seed=7, vocab_size=V),
             "fixed_sampler": lambda: mlm.mask_tokens(ids, ratio, seed=7)}
    alone_t = {k: [] for k in alone}
    for fn in alone.values():
        fn()
    for _ in range(a.windows):
        for k, fn in alone.items():
            alone_t[k].append(timed(fn, 10 * a.iters))
    r3 = lambda t: [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]
    line = json.dumps({"tool": "bench_mlm_labels", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "layers": 12, "heads": 12, "hidden": 768,
                       "vocab": V, "batch": B, "S": S, "tokens": B * S, "rows_a_b": count, "mlm_probability": p, "capacity_c_d": cap,
                       "labelled_c": int((lab_c != -100).sum()), "live_keys_d": int(mask.sum()), "iters": a.iters, "windows": a.windows,
                       "step_ms_median_min_max": {k: r3(t) for k, t in times.items()}, "alone_ms_median_min_max": {k: r3(t) for k, t in alone_t.items()},
                       "label_overflow": int(model.label_overflow), "peak_bytes": int(torch.cuda.max_memory_allocated())})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
