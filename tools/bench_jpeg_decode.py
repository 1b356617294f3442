"""Time of the device JPEG decode (clibd_jpeg_decode_u8, csrc/jpeg.hip) against the host path it replaces.

    python tools/bench_jpeg_decode.py [--batch 2048] [--steps 5] [--rounds 2] [--threads 16] [--skip-lora] [--out profiles/jpeg_decode.log]

The batch is `batch` images of 256 x 341, quality 90, 4:2:0 (PIL's encoder, 256 distinct images repeated).  After a warm-up:
  1. clibd_jpeg_decode_u8 alone by device events (median of five windows): its entropy phase (memset + Huffman kernel), its
     reconstruction phase (IDCT + colour kernels), and both; the bytes that cross to the device in the two forms of a batch.
  2. the host's share of a batch, wall clock, in alternating runs: `pack(decode="host")` (PIL decode + pack on `threads` threads: the
     path of the parent commit, whose code this tree leaves as it was) against `pack(decode="device")` (plan + copy), and `apply` on
     either batch (H2D copies, decode, status read-back, transform), synchronised.
  3. the JPEG-fed LoRA step (ViT-B/16 + BarcodeBERT, `batch` pairs; tools/bench_augment.py's run) with the loader in either form,
     `rounds` alternating runs of `steps` steps each, beside the synthetic step.
Records, not gates.  Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _jpegs(n, h=256, w=341, seed=2, distinct=256):
    import io

    from PIL import Image

    from tools.bench_augment import _images

    enc = []
    for a in _images(min(n, distinct), h, w, seed):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=90, subsampling=2)
        enc.append(buf.getvalue())
    return [enc[i % len(enc)] for i in range(n)]


def device_ms(fn, iters=10, windows=5):
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


def kernel_times(enc, dev):
    import numpy as np
    import torch

    from clibd_amd import augment as A
    from clibd_amd import ops

    packed, sizes = A._pack_device(enc)
    head = packed["plans"][:, :A._PLAN_HEAD.itemsize].contiguous().numpy().view(A._PLAN_HEAD).reshape(-1)
    assert (head["reason"] == 0).all()
    total_blocks = int(head["blocks"].astype(np.int64).sum())
    jpeg, plans, offsets = packed["jpeg"].to(dev), packed["plans"].to(dev), packed["offsets"].to(dev)
    out = torch.empty((int(packed["offsets"][-1]),), dtype=torch.uint8, device=dev)
    ws = torch.empty((int(ops._lib.load().clibd_jpeg_workspace_bytes(total_blocks)),), dtype=torch.uint8, device=dev)
    status = torch.empty((len(enc),), dtype=torch.int32, device=dev)

    def run(phases):
        ops.jpeg_decode(jpeg, plans, offsets, out, total_blocks, status=status, workspace=ws, phases=phases)

    run(3)
    torch.cuda.synchronize()
    assert not status.any().item()
    want, _, _ = A.decode_images(enc[:64], pin=False)
    assert torch.equal(out[:want.numel()].cpu(), want)
    t_entropy, t_recon, t_both = device_ms(lambda: run(1)), device_ms(lambda: run(2)), device_ms(lambda: run(3))
    B = len(enc)
    return {"entropy_phase_device_ms": round(t_entropy, 3), "reconstruction_phase_device_ms": round(t_recon, 3), "decode_device_ms": round(t_both, 3),
            "decode_images_per_s": round(B / t_both * 1e3), "compressed_h2d_mb": round(jpeg.numel() / 1e6, 1),
            "plans_h2d_mb": round(plans.numel() / 1e6, 1), "decoded_h2d_mb": round(out.numel() / 1e6, 1), "workspace_mb": round(ws.numel() / 1e6, 1),
            "total_blocks": total_blocks}


def host_share(enc, threads, dev, rounds):
    import torch

    from clibd_amd import augment as A

    res = {"host": {"pack_ms": [], "apply_ms": []}, "device": {"pack_ms": [], "apply_ms": []}}
    for r in range(rounds + 1):                       # round 0 warms both forms up
        for form in ("host", "device"):
            t0 = time.perf_counter()
            packed = A.pack(enc, train=True, generator=torch.Generator().manual_seed(7), threads=threads, decode=form)
            t1 = time.perf_counter()
            A.apply(packed, dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r:
                res[form]["pack_ms"].append(round((t1 - t0) * 1e3, 1))
                res[form]["apply_ms"].append(round((t2 - t1) * 1e3, 1))
    for form in res:
        res[form]["pack_images_per_s"] = round(len(enc) / statistics.median(res[form]["pack_ms"]) * 1e3)
    return res


def lora_runs(enc, steps, threads, dev, rounds):
    import torch

    from clibd_amd import augment as A
    from clibd_amd.data import DevicePrefetcher, synthetic_batch
    from clibd_amd.train import Trainer, scale_learning_rate
    from tools.bench_deterministic import build

    b = len(enc)
    model = build(dev, full=False)
    tr = Trainer(model, lr=scale_learning_rate(1e-3, b, world_size=1), world_size=1, rank=0, all_gather=True)
    syn = synthetic_batch(b, dev, seed=42, rank=0, with_text=False)
    for _ in range(2):
        tr.step(syn["image"], syn["dna"], None, syn["labels"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(syn["image"], syn["dna"], None, syn["labels"])
    torch.cuda.synchronize()
    out = {"batch": b, "steps": steps, "threads": threads, "synthetic_step_ms": round((time.perf_counter() - t0) / steps * 1e3, 2),
           "jpeg_fed_step_ms": {"host": [], "device": []}}
    dna, labels = syn["dna"].cpu().pin_memory(), syn["labels"].cpu().pin_memory()
    g = torch.Generator().manual_seed(7)

    def batches(n, form):
        for _ in range(n):
            yield {"image": A.pack(enc, train=True, generator=g, threads=threads, decode=form), "dna": dna, "labels": labels}

    warm = 2
    for _ in range(rounds):
        for form in ("host", "device"):
            it = DevicePrefetcher(batches(warm + steps, form), dev)
            for _ in range(warm):
                bt = next(it)
                tr.step(A.apply(bt["image"], dev), bt["dna"], None, bt["labels"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for bt in it:
                loss = tr.step(A.apply(bt["image"], dev), bt["dna"], None, bt["labels"])
            torch.cuda.synchronize()
            out["jpeg_fed_step_ms"][form].append(round((time.perf_counter() - t0) / steps * 1e3, 2))
            assert torch.isfinite(loss).item()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-lora", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    enc = _jpegs(a.batch)
    rec = {"tool": "bench_jpeg_decode", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "batch": a.batch, "image": "256x341 q90 4:2:0",
           "mean_stream_bytes": round(sum(len(e) for e in enc) / len(enc))}
    rec["kernels"] = kernel_times(enc, dev)
    print(json.dumps(rec["kernels"]), flush=True)
    rec["host_share"] = host_share(enc, a.threads, dev, a.rounds)
    print(json.dumps(rec["host_share"]), flush=True)
    if not a.skip_lora:
        rec["lora"] = lora_runs(enc, a.steps, a.threads, dev, a.rounds)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
