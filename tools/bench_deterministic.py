"""Cost of the deterministic training mode (SimpleCLIP.set_deterministic) on one GPU.

    python tools/bench_deterministic.py [--batch 2048] [--steps 5] [--warmup 3] [--pairs 3] [--out profiles/]

1. Full fine-tune step (bench.py --full-finetune configuration: ViT-B/16 + BarcodeBERT, every parameter trainable, global batch 2048 on one
   GPU): the switch off and on in `pairs` interleaved pairs of timed blocks on the same model and trainer, each block `steps` device-
   synchronised steps after warm-up.
2. The LoRA metric step (BASELINE.json metric configuration, B = 2048) with the switch on, and off for reference, the same way.
Prints one JSON line and writes it to <out>/deterministic_mode.log."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(dev, full: bool):
    import torch

    from clibd_amd.model import CLIBDDNAEncoder, CLIBDImageEncoder, SimpleCLIP, create_vit, load_pre_trained_bioscan_bert

    torch.manual_seed(42)
    image_enc = CLIBDImageEncoder(create_vit("vit_base_patch16_224"), r=4, num_classes=768)
    dna_enc = CLIBDDNAEncoder(load_pre_trained_bioscan_bert(None), r=4, num_classes=768)
    model = SimpleCLIP(image_enc, dna_enc, None).to(dev)
    with torch.no_grad():
        for enc in (image_enc, dna_enc):
            for wb in enc.w_Bs:
                wb.weight.normal_(0, 0.02)
    if full:
        for p in model.parameters():
            p.requires_grad_(True)
    return model


def timed_pairs(model, trainer, batch, steps, warmup, pairs, modes):
    import torch

    def block(on):
        model.set_deterministic(on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = trainer.step(batch["image"], batch["dna"], None, batch["labels"])
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        return (time.perf_counter() - t0) / steps * 1e3

    for on in modes:   # warm-up of both modes (workspaces, weight images)
        model.set_deterministic(on)
        for _ in range(warmup):
            trainer.step(batch["image"], batch["dna"], None, batch["labels"])
    torch.cuda.synchronize()
    out = {("on" if on else "off"): [] for on in modes}
    for _ in range(pairs):
        for on in modes:
            out["on" if on else "off"].append(round(block(on), 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default="profiles/")
    args = ap.parse_args()

    import torch

    from clibd_amd.build import csrc_hash
    from clibd_amd.data import synthetic_batch
    from clibd_amd.train import Trainer, scale_learning_rate

    dev = torch.device("cuda:0")
    b = args.batch
    batch = synthetic_batch(b, dev, seed=42, rank=0, with_text=False)
    res = {"tool": "tools/bench_deterministic.py", "csrc_hash": csrc_hash(), "device": torch.cuda.get_device_name(0), "batch": b,
           "steps_per_block": args.steps, "warmup": args.warmup, "pairs": args.pairs}

    model = build(dev, full=True)
    tr = Trainer(model, lr=scale_learning_rate(1e-3, b, world_size=1), world_size=1, rank=0, all_gather=True)
    ff = timed_pairs(model, tr, batch, args.steps, args.warmup, args.pairs, (False, True))
    med = lambda v: sorted(v)[len(v) // 2]
    res["full_finetune_ms"] = dict(ff, median_off=med(ff["off"]), median_on=med(ff["on"]),
                                   overhead_pct=round(100.0 * (med(ff["on"]) / med(ff["off"]) - 1.0), 2))
    del model, tr
    torch.cuda.empty_cache()

    model = build(dev, full=False)
    tr = Trainer(model, lr=scale_learning_rate(1e-3, b, world_size=1), world_size=1, rank=0, all_gather=True)
    lo = timed_pairs(model, tr, batch, args.steps, args.warmup, args.pairs, (False, True))
    res["lora_metric_ms"] = dict(lo, median_off=med(lo["off"]), median_on=med(lo["on"]),
                                 overhead_pct=round(100.0 * (med(lo["on"]) / med(lo["off"]) - 1.0), 2))
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "deterministic_mode.log"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
