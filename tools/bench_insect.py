"""Time of the INSECT / BZSL workflow's kernels and steps (clibd_amd.insect) at the workflow's shapes.

    python tools/bench_insect.py [--batch 300] [--classes 1213] [--skip-step] [--skip-large] [--out profiles/insect.log]

As medians of 5 windows of device-event time, after a warm-up:
  1. clibd_class_mean_f32 (the whole entry: histogram, scan, fill, sort, chains) at the nominal INSECT shape N = 21 212 rows,
     C = 1 213 classes, D = 768, with the [D, C] table layout, and at N = 2^20, C = 8 192, D = 768 (3 GiB of features);
  2. clibd_logits_topk (k = 5) over 16 000 x 1 213 logits;
  3. one joint fine-tuning step (ViT-B/16 + BarcodeBERT under LoRA, two 1 213-way heads, one FusedAdamW) at batch 300, next to the
     image-only and the DNA-only step of the same classifiers.  The towers of the joint step run one after the other on the current
     stream: the three figures are the baseline of any later change that overlaps them.
Random features with uniformly drawn labels.  Records, not gates: there is no parent to compare with.
Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_ms(fn, iters=20, windows=5):
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
    return statistics.median(out)


def time_class_mean(N, C, D, dev, gen, iters):
    import torch

    from clibd_amd import ops

    x = torch.randn(N, D, device=dev)
    labels = torch.randint(0, C, (N,), generator=gen).to(torch.int32).to(dev)
    out = torch.empty((D, C), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    run = lambda: ops.class_mean(x, labels, C, transposed=True, out=out, error=err)
    run()
    torch.cuda.synchronize()
    ms = device_ms(run, iters=iters)
    return ms, (N * D * 4 + N * 4) / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=300)
    ap.add_argument("--classes", type=int, default=1213)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from clibd_amd import insect as I
    from clibd_amd import ops
    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    C = a.classes
    rec = {"tool": "bench_insect", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "classes": C}

    ms, gbs = time_class_mean(21212, C, 768, dev, gen, 20)
    rec.update(class_mean_insect_device_ms=round(ms, 4), class_mean_insect_read_gb_s=round(gbs, 1), class_mean_insect_shape=[21212, C, 768])
    if not a.skip_large:
        ms, gbs = time_class_mean(1 << 20, 8192, 768, dev, gen, 3)
        rec.update(class_mean_large_device_ms=round(ms, 4), class_mean_large_read_gb_s=round(gbs, 1), class_mean_large_shape=[1 << 20, 8192, 768])
        torch.cuda.empty_cache()

    logits = torch.randn(16000, C, device=dev)
    ops.logits_topk(logits, 5)
    ms = device_ms(lambda: ops.logits_topk(logits, 5))
    rec.update(logits_topk_device_ms=round(ms, 4), logits_topk_rows=16000, logits_topk_read_gb_s=round(16000 * C * 4 / (ms * 1e-3) / 1e9, 1))

    if not a.skip_step:
        from clibd_amd.model import CLIBDDNAEncoder, CLIBDImageEncoder, SimpleCLIP, create_vit, load_pre_trained_bioscan_bert
        from clibd_amd.optim import FusedAdamW

        torch.manual_seed(42)
        image_enc = CLIBDImageEncoder(create_vit("vit_base_patch16_224"), r=4, num_classes=768)
        dna_enc = CLIBDDNAEncoder(load_pre_trained_bioscan_bert(None), r=4, num_classes=768)
        model = SimpleCLIP(image_enc, dna_enc, None).to(dev)
        with torch.no_grad():   # B != 0, as in bench.py: B = 0 would make half the LoRA backward trivially zero
            for enc in (image_enc, dna_enc):
                for wb in enc.w_Bs:
                    wb.weight.normal_(0, 0.02)
        ic, dc = I.build_classifiers(model, C, 768, dev)
        ic.train()
        dc.train()
        b = a.batch
        images = torch.randn(b, 3, 224, 224, generator=gen).to(dev)
        ids = torch.randint(5, 1027, (b, 133), generator=gen).to(dev)
        target = torch.randint(0, C, (b,), generator=gen).to(dev)
        crit = I.CrossEntropyLoss()

        def stepper(mods):
            opt = FusedAdamW(I.combined_parameters(*mods), lr=1e-3)

            def step():
                opt.zero_grad()
                loss = None
                for m in mods:
                    term = crit(m(images if m is ic else ids), target)
                    loss = term if loss is None else loss + term
                loss.backward()
                opt.step()

            return step

        for name, mods in (("joint", (ic, dc)), ("image_only", (ic,)), ("dna_only", (dc,))):
            step = stepper(mods)
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            rec[f"{name}_step_device_ms"] = round(device_ms(step, iters=3), 3)
        rec["step_batch"] = b

    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
