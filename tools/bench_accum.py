"""Time of the masked-LM pre-training step with accumulation windows (clibd_amd.mlm, clibd_amd.optim) beside the plain
step, on one MI355X.

    python tools/bench_accum.py [--batch 256] [--iters 10] [--windows 5] [--out profiles/accum.log]

BERT-base BarcodeBERT (12 layers x 12 heads of 64, hidden 768, k = 5: vocabulary 1027, S = 133), train mode, tied weights, FusedAdamW.
One process; the three forms ALTERNATE inside every window (a, b, c, a, b, ...), device events, medians over the windows:
  a  the plain step written out as the parent's pretrain_step ran it: zero_grad, mask_tokens(ratio 0.5), model(masked, rows, targets,
     n_valid), backward, optimizer.step();
  b  mlm.pretrain_step with accumulation_steps = 1 on this tree (the same launches, through the new driver code);
  c  one window of 4 micro-steps of the same batch size, mlm.pretrain_step(accumulation_steps=4): sum-mode cross-entropy, the three aux
     adds, and on the fourth the norm with the device divisor plus the grouped update; reported per window and per micro-step.
a and b share one model and optimizer; c has its own (its optimizer carries the divisor slot).  And alone, on the bucket of this model:
ops.grad_norm, ops.grad_norm_div, the plain update and the grouped update reading the record.
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
        raise RuntimeError("bench_accum.py measures on an MI355X: no GPU found")
    from clibd_amd import mlm, ops
    from clibd_amd.build import csrc_hash
    from clibd_amd.model import BertConfigLite, BertForMaskedLM
    from clibd_amd.optim import FusedAdamW

    dev = torch.device("cuda:0")
    V, B, S, ratio, K = 1027, a.batch, 133, 0.5, 4

    def build(k):
        torch.manual_seed(0)
        model = mlm.BarcodeBERTForPreTraining(BertForMaskedLM(BertConfigLite(vocab_size=V, max_position_embeddings=256))).to(dev).train()
        opt = FusedAdamW(model.parameters(), lr=1e-4, accumulation_steps=k)
        model.attach(opt)
        return model, opt

    model, opt = build(1)
    model_k, opt_k = build(K)
    g = torch.Generator().manual_seed(1)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1).to(dev)

    def step_a():
        opt.zero_grad()
        masked, rows, targets, n_valid = mlm.mask_tokens(ids, ratio, 7)
        loss, _ = model(masked, rows, targets, n_valid)
        loss.backward()
        opt.step()

    def step_b():
        mlm.pretrain_step(model, ids, opt, ratio, seed=7, accumulation_steps=1)

    def step_c():
        for _ in range(K):
            mlm.pretrain_step(model_k, ids, opt_k, ratio, seed=7, accumulation_steps=K)

    forms = {"a_plain_step": step_a, "b_pretrain_step_k1": step_b, "c_window_of_4": step_c}
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert opt.divisor_slot is None and opt_k.divisor_slot == mlm.AUX_COUNT and not opt_k.window_open
    times = {k: [] for k in forms}
    for _ in range(a.windows):
        for k, fn in forms.items():
            times[k].append(timed(fn, a.iters))
    n = opt.flat_g.numel()
    rec = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = ops.grad_norm_workspace(n, dev)
    div = torch.tensor([float(B * (S - 1) // 2)], dtype=torch.float32, device=dev)
    table = [(0, 1e-4, 1e-2)]
    alone = {"grad_norm": lambda: ops.grad_norm(opt.flat_g, rec, ws, 1.0, 1.0, True),
             "grad_norm_div": lambda: ops.grad_norm_div(opt.flat_g, rec, ws, div, 1.0, 1.0, True),
             "adamw_step": lambda: ops.adamw_step(opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 5, 1.0),
             "adamw_step_groups_record": lambda: ops.adamw_step_groups(opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq, table, 0.9, 0.999, 1e-8, 5, 1.0, rec)}
    alone_t = {k: [] for k in alone}
    for fn in alone.values():
        fn()
    for _ in range(a.windows):
        for k, fn in alone.items():
            alone_t[k].append(timed(fn, 10 * a.iters))
    r3 = lambda t: [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]
    steps = {k: r3(t) for k, t in times.items()}
    steps["c_per_micro_step"] = r3([t / K for t in times["c_window_of_4"]])
    line = json.dumps({"tool": "bench_accum", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "layers": 12, "heads": 12, "hidden": 768,
                       "vocab": V, "batch": B, "S": S, "tokens": B * S, "accumulation_steps_c": K, "bucket_floats": n, "iters": a.iters,
                       "windows": a.windows, "step_ms_median_min_max": steps, "alone_ms_median_min_max": {k: r3(t) for k, t in alone_t.items()},
                       "updates_a_b": opt.step_count, "updates_c": opt_k.step_count, "peak_bytes": int(torch.cuda.max_memory_allocated())})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
