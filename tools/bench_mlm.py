"""Time of one masked-k-mer pre-training step (clibd_amd.mlm) on one MI355X, train mode, FusedAdamW.

    python tools/bench_mlm.py [--shapes base,6x6,4x4] [--batch 256] [--ratio 0.5] [--iters 10] [--windows 5] [--out profiles/mlm.log]

Shapes (hidden 768, intermediate 3072):
  base  12 layers x 12 heads (64 wide),  k = 5: vocabulary 1027, S = 133     the BERT-base BarcodeBERT
  6x6    6 layers x  6 heads (128 wide), k = 4: vocabulary 259,  S = 166     the newer checkpoints
  4x4    4 layers x  4 heads (192 wide), k = 4: vocabulary 259,  S = 166
Per shape, after a warm-up, device-event medians over `windows` windows of `iters` back-to-back repeats of
  step     mask_tokens + forward + backward + optimizer step (pretrain_step), random k-mer ids, tied weights;
  sampler  mask_tokens alone;
  head     the vocabulary head alone on a fixed top hidden state: gather, transform, LayerNorm, decoder, cross-entropy, then their
           backward and the scatter (the gradients go into a scratch bucket);
  tower    the BertTower recording forward + full backward alone, fed a fixed bf16 gradient of the top hidden state;
  adamw    the optimizer's one launch.
Records, not gates: the pre-training step has no parent to compare with.  Prints one JSON line per shape (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"base": dict(layers=12, heads=12, k=5, S=133), "6x6": dict(layers=6, heads=6, k=4, S=166), "4x4": dict(layers=4, heads=4, k=4, S=166)}


def device_ms(fn, iters, windows):
    import torch

    out = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters)
    return statistics.median(out), min(out), max(out)


def bench_shape(name, a):
    import torch

    from clibd_amd import mlm
    from clibd_amd.build import csrc_hash
    from clibd_amd.engine import GradBucket
    from clibd_amd.model import BertConfigLite, BertForMaskedLM
    from clibd_amd.optim import FusedAdamW

    sh = SHAPES[name]
    dev = torch.device("cuda:0")
    V, B, S = 4 ** sh["k"] + 3, a.batch, sh["S"]
    torch.manual_seed(0)
    model = mlm.BarcodeBERTForPreTraining(BertForMaskedLM(BertConfigLite(vocab_size=V, num_hidden_layers=sh["layers"], num_attention_heads=sh["heads"],
                                                                         max_position_embeddings=256))).to(dev).train()
    opt = FusedAdamW(model.parameters(), lr=1e-4)
    model.attach(opt)
    g = torch.Generator().manual_seed(1)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1).to(dev)

    def step():
        mlm.pretrain_step(model, ids, opt, a.ratio)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t_step = device_ms(step, a.iters, a.windows)
    t_mask = device_ms(lambda: mlm.mask_tokens(ids, a.ratio), 10 * a.iters, a.windows)

    masked, rows, targets, n_valid = mlm.mask_tokens(ids, a.ratio, seed=7)
    tw = model.tower()
    tw.training = True
    x_top, _ = tw._forward((masked, None, None), True)
    x_top = x_top.clone()
    bucket = GradBucket(model.trainable_params())
    one = torch.ones((), device=dev)

    def head():
        loss, correct, st = model._head_forward(x_top, rows, targets, n_valid)
        return model._head_backward(one, st, bucket.views)

    dx = head().clone()

    def tower():
        _, state = tw._forward((masked, None, None), True)
        tw._backward(dx, state, bucket.views)

    head(); tower()
    torch.cuda.synchronize()
    t_head, t_tower, t_opt = device_ms(head, a.iters, a.windows), device_ms(tower, a.iters, a.windows), device_ms(opt.step, 10 * a.iters, a.windows)
    r3 = lambda t: [round(x, 3) for x in t]
    return {"tool": "bench_mlm", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "shape": name, **sh, "hidden": 768, "vocab": V, "batch": B,
            "ratio": a.ratio, "masked_rows": int(rows.numel()), "tokens": B * S, "parameters": int(opt.flat_p.numel()), "iters": a.iters,
            "windows": a.windows, "step_ms_median_min_max": r3(t_step), "sampler_ms": r3(t_mask), "head_fwd_bwd_ms": r3(t_head),
            "tower_fwd_bwd_ms": r3(t_tower), "adamw_ms": r3(t_opt),
            "sampler_plus_head_share_of_step": round((t_mask[0] + t_head[0]) / t_step[0], 4),
            "peak_bytes": int(torch.cuda.max_memory_allocated())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="base,6x6,4x4")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("bench_mlm.py measures on an MI355X: no GPU found")
    for name in a.shapes.split(","):
        line = json.dumps(bench_shape(name, a))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
