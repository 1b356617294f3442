"""Time of the linear-probe classifier (clibd_amd.method_linear) at the reference's shape.

    python tools/bench_method_linear.py [--classes 916] [--dim 768] [--batch 150] [--seen 8000] [--unseen 8000] [--unseen-keys 9118]
                                        [--reps 3] [--out profiles/method_linear.log]

C = 916 classes, D = 768, batch 150 (the reference's fine_tuning_set).  After a warm-up it times, as medians of 5 windows of device-event
time,
  1. the head + cross-entropy forward and backward of one training step (clibd_linear_f32_fwd, clibd_ce_rows_fwd, clibd_ce_rows_bwd,
     clibd_linear_f32_bwd with dx, dw and db), and the forward pair alone;
  2. clibd_softmax_topk (k = 5) on the logits of all seen + unseen queries;
and, as the best of --reps wall-clock runs, the whole `classifier_seen_unseen_from_features` call (softmax top-k, the image -> DNA search,
the sweep over 1 001 thresholds, merge, scoring) with label lists and with index arrays.  Synthetic features around species centres
shared by the image and the DNA modality; the head is the matrix of the seen species' normalised centres times a temperature, so the
classifier is right most of the time without being trained here.  Records, not gates: there is no parent to compare with.
Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K_LIST = [1, 3, 5]


def taxonomy(s: int) -> dict:
    return {"order": f"o{s // 500}", "family": f"f{s // 60}", "genus": f"g{s // 4}", "species": f"s{s}"}


def make_split(n, species, centers, gen, dev, noise):
    import torch

    from clibd_amd import ops

    sp = species[torch.randint(0, len(species), (n,), generator=gen)]
    x = centers[sp.to(dev)] + noise * torch.randn(n, centers.shape[1], generator=gen).to(dev)
    return ops.l2norm_fwd(x.contiguous())[0], sp, [taxonomy(int(s)) for s in sp.tolist()]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=916)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=150)
    ap.add_argument("--seen", type=int, default=8000)
    ap.add_argument("--unseen", type=int, default=8000)
    ap.add_argument("--unseen-keys", type=int, default=9118)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from clibd_amd import method_linear as ML
    from clibd_amd import ops
    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    C, D = a.classes, a.dim
    S = 2 * C
    centers = torch.randn(S, D, generator=gen).to(dev)
    seen_sp, unseen_sp = torch.arange(C), torch.arange(C, S)
    seen_q, seen_t, seen_gt = make_split(a.seen, seen_sp, centers, gen, dev, 1.5)
    unseen_q, _, unseen_gt = make_split(a.unseen, unseen_sp, centers, gen, dev, 1.5)
    unseen_keys, _, unseen_keys_label = make_split(a.unseen_keys, unseen_sp, centers, gen, dev, 1.2)
    w = (ops.l2norm_fwd(centers[:C].contiguous())[0] * 12.0).contiguous()
    b = torch.zeros(C, device=dev)
    class_labels = [taxonomy(s) for s in range(C)]

    # ---- one training step's head + CE
    x = seen_q[: a.batch].contiguous()
    t = seen_t[: a.batch].to(dev)

    def fwd():
        logits = ops.linear_f32_fwd(x, w, b)
        return logits, ops.ce_rows_fwd(logits, t)

    def fwd_bwd():
        logits, (_, lse) = fwd()
        ops.linear_f32_bwd(ops.ce_rows_bwd(logits, t, lse), x, w)

    fwd_bwd()
    torch.cuda.synchronize()
    t_fwd, t_step = device_ms(fwd), device_ms(fwd_bwd)

    # ---- softmax top-k over every query, then the whole method
    seen_logits, unseen_logits = ops.linear_f32_fwd(seen_q, w, b), ops.linear_f32_fwd(unseen_q, w, b)
    all_logits = torch.cat([seen_logits, unseen_logits])
    ops.softmax_topk(all_logits, 5)
    t_topk = device_ms(lambda: ops.softmax_topk(all_logits, 5))

    def whole(with_predictions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ML.classifier_seen_unseen_from_features(seen_logits, unseen_logits, class_labels, seen_q, unseen_q, unseen_keys, unseen_keys_label,
                                                      seen_gt, unseen_gt, K_LIST, with_predictions=with_predictions)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    whole(True)                                                               # warm-up
    t_pred = min(whole(True)[0] for _ in range(a.reps))
    runs = [whole(False) for _ in range(a.reps)]
    t_idx, (seen_out, unseen_out) = min(r[0] for r in runs), runs[0][1]

    rec = {"tool": "bench_method_linear", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "classes": C, "D": D, "batch": a.batch,
           "seen": a.seen, "unseen": a.unseen, "unseen_keys": a.unseen_keys, "thresholds": 1001, "k_list": K_LIST,
           "head_ce_fwd_device_ms": round(t_fwd, 4), "head_ce_fwd_bwd_device_ms": round(t_step, 4),
           "softmax_topk_device_ms": round(t_topk, 4), "softmax_topk_rows": int(all_logits.shape[0]),
           "classifier_seen_unseen_from_features_s_with_predictions": round(t_pred, 4),
           "classifier_seen_unseen_from_features_s_index_arrays": round(t_idx, 4), "best_threshold": float(seen_out["best_threshold"]),
           "top1_species_seen": seen_out["micro_acc"][1]["species"], "top1_species_unseen": unseen_out["micro_acc"][1]["species"]}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
