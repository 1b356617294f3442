"""Time and peak memory of the chunked contrastive step (clibd_amd.chunked, Trainer(chunk_size=...)) beside the plain step, on one
MI355X.

    python tools/bench_chunked_step.py [--batch 2048] [--chunks 1024,512,256] [--big 4096,8192] [--big-chunk 1024] [--iters 4] [--windows 2]
                                       [--out profiles/chunked_step.log]

The metric's configuration (bench.py: ViT-B/16 + BarcodeBERT, LoRA r = 4, image + DNA, train mode so the DNA tower's dropout is on, synthetic
batch), one process, one model; a Trainer per form, one after the other (a Trainer re-homes the model's parameters into its own bucket):
  plain             Trainer.step as it always was;
  chunk_size = c    the two-pass step for every c of --chunks, replay guard on (the default);
  chunk_size = c, replay_guard=False   for the first c only: what the guard's compare costs.
Per form: two warm-up steps, then `windows` windows of `iters` steps between device events (median, min, max of the windows' ms per step), and
torch.cuda.max_memory_allocated over the timed steps (reset after the warm-up) beside what was allocated before them.
Then the batches of --big with chunk_size --big-chunk, chunked only.  Before each, the peak is predicted — what is allocated with the batch on the
device, plus the peak a chunk of that size added at --batch, plus the embedding caches (cache, dE and the loss's three copies: 5 x modalities x b x D
fp32) and the loss workspaces for b rows — and compared with the free memory; a configuration that does not fit under 90 % of it is skipped and
reported as such.  No form is run that is expected to run out of memory.
Records, not gates.  Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--chunks", default="1024,512,256")
    ap.add_argument("--big", default="4096,8192")
    ap.add_argument("--big-chunk", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("bench_chunked_step.py measures on an MI355X: no GPU found")
    from clibd_amd import _lib
    from clibd_amd.build import csrc_hash
    from clibd_amd.data import synthetic_batch
    from clibd_amd.model import CLIBDDNAEncoder, CLIBDImageEncoder, SimpleCLIP, create_vit, load_pre_trained_bioscan_bert
    from clibd_amd.train import Trainer, scale_learning_rate

    dev = torch.device("cuda:0")
    D, M = 768, 2
    torch.manual_seed(42)
    image_enc = CLIBDImageEncoder(create_vit("vit_base_patch16_224"), r=4, num_classes=D)
    dna_enc = CLIBDDNAEncoder(load_pre_trained_bioscan_bert(None), r=4, num_classes=D)
    model = SimpleCLIP(image_enc, dna_enc, None).to(dev)
    with torch.no_grad():
        for enc in (image_enc, dna_enc):
            for wb in enc.w_Bs:
                wb.weight.normal_(0, 0.02)
    model.train(True)

    def measure(batch, b, chunk, guard=True, warmup=2, iters=a.iters, windows=a.windows):
        tr = Trainer(model, lr=scale_learning_rate(1e-3, b), chunk_size=chunk, replay_guard=guard)
        step = lambda: tr.step(batch["image"], batch["dna"], batch["text"], batch["labels"])
        for _ in range(warmup):
            loss = step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(windows):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                loss = step()
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e) / iters)
        peak = torch.cuda.max_memory_allocated()
        rec = {"batch": b, "chunk_size": chunk, "replay_guard": bool(guard) if chunk is not None else None,
               "ms_per_step_median_min_max": [round(statistics.median(times), 2), round(min(times), 2), round(max(times), 2)],
               "peak_bytes": int(peak), "allocated_before_bytes": int(base), "peak_above_before_bytes": int(peak - base), "loss": round(float(loss), 5),
               "replay_mismatch": None if tr.replay_mismatch is None else int(tr.replay_mismatch), "updates": tr.optimizer.step_count}
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del tr
        return rec

    b = a.batch
    chunks = [int(c) for c in a.chunks.split(",") if c]
    batch = synthetic_batch(b, dev, seed=42, rank=0, with_text=False)
    rows = [measure(batch, b, None)]
    for c in chunks:
        rows.append(measure(batch, b, c))
    if chunks:
        rows.append(measure(batch, b, chunks[0], guard=False))
    plain_ms = rows[0]["ms_per_step_median_min_max"][0]
    for r in rows:
        r["time_over_plain"] = round(r["ms_per_step_median_min_max"][0] / plain_ms, 3)
        r["peak_over_plain"] = round(r["peak_bytes"] / rows[0]["peak_bytes"], 3)
    # what a chunk of --big-chunk samples adds to the allocation: measured at --batch
    ref = next((r for r in rows if r["chunk_size"] == a.big_chunk and r["replay_guard"]), None) or measure(batch, b, a.big_chunk)
    chunk_added = ref["peak_above_before_bytes"]
    del batch
    big = []
    lib = _lib.load()
    for bb in [int(x) for x in a.big.split(",") if x]:
        gc.collect()
        torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info()
        inputs = bb * (3 * 224 * 224 * 4 + 133 * 8 + 8)
        caches = 5 * M * bb * D * 4
        loss_ws = 2 * int(lib.clibd_softce_workspace_bytes(bb, bb, D))            # image -> DNA and DNA -> image
        need = inputs + chunk_added + caches + loss_ws
        rec = {"batch": bb, "chunk_size": a.big_chunk, "free_bytes": int(free), "total_bytes": int(total),
               "predicted_peak_bytes": int(torch.cuda.memory_allocated() + need), "predicted_added_bytes": {"inputs": inputs, "chunk": chunk_added, "caches": caches, "loss_workspaces": loss_ws, "sum": need}}
        if need > 0.9 * free:
            rec["skipped"] = "predicted peak above 90 % of the free memory"
            print(json.dumps(rec), file=sys.stderr, flush=True)
        else:
            batch = synthetic_batch(bb, dev, seed=42, rank=0, with_text=False)
            rec.update(measure(batch, bb, a.big_chunk, warmup=1, iters=max(1, a.iters // 2), windows=a.windows))
            del batch
        big.append(rec)
    line = json.dumps({"tool": "bench_chunked_step", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "towers": "image+dna", "lora_r": 4,
                       "train_mode": True, "iters": a.iters, "windows": a.windows, "at_metric_batch": rows, "larger_batches": big})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
