"""Cost of the device image transforms (clibd_image_transform_u8) and of feeding the training step from JPEG bytes.

    python tools/bench_augment.py [--batch 2048] [--reps 20] [--steps 5] [--out profiles/]

1. Device time of the training and eval transforms at `batch` for 256x341, 512x683 and 1024x1365 sources (events around `reps` launches
   after warm-up), with the bytes each moves and the HBM bound at 6.3 TB/s (the measured copy rate).
2. Host rates with 16 threads: PIL decode + pack (decode_images), and the reference's per-image chain restated with torch CPU ops
   (tests/augment_reference.py), i.e. what the reference's DataLoader workers pay.
3. One LoRA metric run (ViT-B/16 + BarcodeBERT, `batch` pairs) fed from JPEG bytes: decode threads -> DevicePrefetcher -> apply ->
   Trainer.step, in ms per step, against the synthetic step of the same run.
Prints one JSON line and appends it to <out>/augment.log."""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
SIZES = [(256, 341), (512, 683), (1024, 1365)]


def _images(n, h, w, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(yy[..., None] * 0.05 + xx[..., None] * 0.03 + np.arange(3))
    return [np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8) for _ in range(n)]


def _jpegs(n, h, w, seed, distinct=64):
    from PIL import Image

    enc = []
    for a in _images(min(n, distinct), h, w, seed):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=90)
        enc.append(buf.getvalue())
    return [enc[i % len(enc)] for i in range(n)]


def device_times(b, reps, dev):
    import torch

    from clibd_amd import augment as A
    from clibd_amd import ops

    rows = []
    for h, w in SIZES:
        data = torch.randint(0, 256, (b * h * w * 3,), dtype=torch.uint8, device=dev)
        sizes = [(h, w)] * b
        for mode, rec in (("train", A.sample_train_params(sizes, torch.Generator().manual_seed(0))), ("eval", A.eval_params(sizes))):
            xf = rec.to(dev)
            ws = torch.empty((int(ops._lib.load().clibd_image_transform_workspace_bytes(b)),), dtype=torch.uint8, device=dev)
            for _ in range(3):
                ops.image_transform(data, xf, ws)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            times = []
            for _ in range(reps):
                e0.record()
                ops.image_transform(data, xf, ws)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            times.sort()
            read, write = b * h * w * 3, b * 224 * 224 * 3 * 4
            extra = 2 * write if mode == "train" else 0     # pre-rotation image: written and read back
            ms = times[len(times) // 2]
            rows.append({"size": f"{h}x{w}", "mode": mode, "ms_median": round(ms, 4), "ms_min": round(times[0], 4), "reps": reps,
                         "GB_moved": round((read + write + extra) / 1e9, 3), "bound_ms": round((read + write + extra) / HBM * 1e3, 4),
                         "share_of_bound": round((read + write + extra) / HBM * 1e3 / ms, 3)})
            del ws
        del data
        torch.cuda.empty_cache()
    return rows


def host_rates(n, threads):
    import torch

    from clibd_amd import augment as A
    from tests import augment_reference as R

    out = {}
    for h, w in SIZES:
        enc = _jpegs(n, h, w, 1)
        A.decode_images(enc[:threads], threads=threads)
        t0 = time.perf_counter()
        data, offsets, sizes = A.decode_images(enc, threads=threads)
        dt = time.perf_counter() - t0
        out[f"decode_pack_{h}x{w}_img_per_s"] = round(n / dt, 1)
        imgs = [data[offsets[i]:offsets[i + 1]].numpy().reshape(h, w, 3) for i in range(min(n, 256))]
        p = A.params_from_uniforms([(h, w)] * len(imgs), A.draw_uniforms(len(imgs), torch.Generator().manual_seed(0)))
        nt = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            def chain(i):
                return R.train_chain(imgs[i], int(p["top"][i]), int(p["left"][i]), int(p["h"][i]), int(p["w"][i]), bool(p["hflip"][i]),
                                     bool(p["vflip"][i]), float(p["angle"][i]))
            with cf.ThreadPoolExecutor(threads) as ex:
                list(ex.map(chain, range(threads)))
                t0 = time.perf_counter()
                list(ex.map(chain, range(len(imgs))))
                dt = time.perf_counter() - t0
        finally:
            torch.set_num_threads(nt)
        out[f"host_chain_{h}x{w}_img_per_s"] = round(len(imgs) / dt, 1)
    return out


def lora_run(b, steps, threads, dev):
    import torch

    from clibd_amd import augment as A
    from clibd_amd.data import DevicePrefetcher, synthetic_batch
    from clibd_amd.train import Trainer, scale_learning_rate
    from tools.bench_deterministic import build

    model = build(dev, full=False)
    tr = Trainer(model, lr=scale_learning_rate(1e-3, b, world_size=1), world_size=1, rank=0, all_gather=True)
    syn = synthetic_batch(b, dev, seed=42, rank=0, with_text=False)
    for _ in range(2):
        tr.step(syn["image"], syn["dna"], None, syn["labels"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = tr.step(syn["image"], syn["dna"], None, syn["labels"])
    torch.cuda.synchronize()
    syn_ms = (time.perf_counter() - t0) / steps * 1e3

    enc = _jpegs(b, 256, 341, 2, distinct=256)
    g = torch.Generator().manual_seed(7)
    decode_ms = []

    def batches(n):
        for _ in range(n):
            t = time.perf_counter()
            img = A.pack(enc, train=True, generator=g, threads=threads)
            decode_ms.append((time.perf_counter() - t) * 1e3)
            yield {"image": img, "dna": syn["dna"].cpu().pin_memory(), "labels": syn["labels"].cpu().pin_memory()}

    warm = 2
    it = DevicePrefetcher(batches(warm + steps), dev)
    for _ in range(warm):
        bt = next(it)
        tr.step(A.apply(bt["image"], dev), bt["dna"], None, bt["labels"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for bt in it:
        loss = tr.step(A.apply(bt["image"], dev), bt["dna"], None, bt["labels"])
    torch.cuda.synchronize()
    real_ms = (time.perf_counter() - t0) / steps * 1e3
    assert torch.isfinite(loss).item()
    return {"batch": b, "steps": steps, "decode_threads": threads, "synthetic_step_ms": round(syn_ms, 2), "jpeg_fed_step_ms": round(real_ms, 2),
            "host_pack_ms_per_batch": sorted(round(x, 1) for x in decode_ms), "decode_keeps_up": real_ms <= 1.03 * syn_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-lora", action="store_true")
    ap.add_argument("--out", default="profiles/")
    args = ap.parse_args()

    import torch

    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    res = {"tool": "tools/bench_augment.py", "csrc_hash": csrc_hash(), "device": torch.cuda.get_device_name(0), "batch": args.batch,
           "hbm_rate_assumed_TBps": HBM / 1e12}
    res["device_transform"] = device_times(args.batch, args.reps, dev)
    print(json.dumps(res["device_transform"]), flush=True)
    res["host_16_threads"] = host_rates(args.host_images, args.threads)
    print(json.dumps(res["host_16_threads"]), flush=True)
    if not args.skip_lora:
        res["lora_jpeg_fed"] = lora_run(args.batch, args.steps, args.threads, dev)
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "augment.log"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
