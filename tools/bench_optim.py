"""Time of the optimizer update with and without clipping and groups (clibd_amd.optim), on one MI355X.

    python tools/bench_optim.py [--iters 100] [--windows 7] [--out profiles/optim.log]

Two flat fp32 buckets: the full fine-tune's size (174 M values: ViT-B/16 + BarcodeBERT, every parameter trainable) and the LoRA run's
(1.48 M values).  One process; the three forms ALTERNATE inside every window (a, b, c, a, b, ...), device events, median (min ... max)
over the windows:
  a  ops.adamw_step — today's single launch, the path `step()` keeps for one group without clipping;
  b  ops.adamw_step_groups alone: two groups (the second a tenth of the bucket, no decay), no record — the float4 kernel;
  c  ops.grad_norm + ops.adamw_step_groups reading its record (max_norm below the norm: clipped; skip on) — a step that clips.
And the norm launch alone.  Bytes are counted from the shapes: the update reads p, g, m, v and writes p, m, v (28 bytes per value), the
norm reads g (4 bytes per value); GB/s = those bytes over the median time.  Records, not gates.  Prints one JSON line per bucket (and
appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BUCKETS = {"full_finetune": 174_000_000, "lora": 1_480_000}


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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("bench_optim.py measures on an MI355X: no GPU found")
    from clibd_amd import ops
    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    for name, n in BUCKETS.items():
        n = (n + 63) // 64 * 64
        gen = torch.Generator(device=dev).manual_seed(0)
        p = torch.randn(n, generator=gen, device=dev) * 0.02
        g = torch.randn(n, generator=gen, device=dev) * 1e-3
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        record = torch.zeros((4,), dtype=torch.int32, device=dev)
        ws = ops.grad_norm_workspace(n, dev)
        second = n // 10 // 64 * 64
        groups = [(0, 1e-4, 1e-2), (n - second, 1e-4, 0.0)]
        hyp = (0.9, 0.999, 1e-8)
        step = [0]

        def form_a():
            step[0] += 1
            ops.adamw_step(p, g, m, v, 1e-4, *hyp, 1e-2, step[0], 1.0)

        def form_b():
            step[0] += 1
            ops.adamw_step_groups(p, g, m, v, groups, *hyp, step[0], 1.0, None)

        def form_c():
            step[0] += 1
            ops.grad_norm(g, record, ws, 1.0, 1.0, True)
            ops.adamw_step_groups(p, g, m, v, groups, *hyp, step[0], 1.0, record)

        def norm_alone():
            ops.grad_norm(g, record, ws, 1.0, 1.0, True)

        forms = {"a_adamw_step": form_a, "b_groups_alone": form_b, "c_norm_and_groups": form_c, "norm_alone": norm_alone}
        iters = a.iters if n > 10_000_000 else 10 * a.iters
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.windows):
            for k, fn in forms.items():
                times[k].append(timed(fn, iters))
        rec = record.cpu()
        nbytes = {"a_adamw_step": 28 * n, "b_groups_alone": 28 * n, "c_norm_and_groups": 32 * n, "norm_alone": 4 * n}
        r3 = lambda t: [round(statistics.median(t), 5), round(min(t), 5), round(max(t), 5)]
        line = json.dumps({"tool": "bench_optim", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "bucket": name, "values": n,
                           "groups": [g0[0] for g0 in groups], "iters": iters, "windows": a.windows,
                           "ms_median_min_max": {k: r3(t) for k, t in times.items()},
                           "gb_per_s_at_median": {k: round(nbytes[k] / statistics.median(t) / 1e6, 1) for k, t in times.items()},
                           "grad_norm": rec.view(torch.float32)[0].item(), "coef": rec.view(torch.float32)[1].item(), "skipped": int(rec[3]),
                           "finite": bool(torch.isfinite(p).all())})
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del p, g, m, v


if __name__ == "__main__":
    main()
