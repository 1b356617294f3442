"""Time of the seen/unseen threshold method (clibd_amd.method_nn) at BIOSCAN-1M's eval shape.

    python tools/bench_method_nn.py [--seen-keys 12000] [--unseen-keys 9118] [--seen 8000] [--unseen 8000] [--thresholds 1000]
                                    [--cpu-thresholds 10] [--reps 3] [--out profiles/method_nn.log]

Synthetic features (D = 768) around species centres shared by the image and the DNA modality (8 000 species; the seen keys are image
embeddings of the first half, the unseen keys DNA embeddings of the second half).  After one warm-up it times
  1. the device threshold search alone: clibd_threshold_sweep_hits over every threshold (m = 5, two segments) + the copy of the
     counts + the host finaliser (harmonic curve, first maximum);
  2. the whole `seen_unseen_from_features` call (two searches, sweep, merge, scoring), with label lists and with index arrays;
  3. the reference's convention restated on the CPU: per threshold and split, a Python list of merged label dicts and the
     top_k_micro_accuracy loops over every k and level, to read micro_acc[1]['species'].  Timed on --cpu-thresholds thresholds spread
     evenly over the grid and scaled to the full grid (the work per threshold does not depend on its value); the hit counts of those
     thresholds are asserted equal to the device's.
Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = ["order", "family", "genus", "species"]
K_LIST = [1, 3, 5]


def taxonomy(s: int) -> dict:
    return {"order": f"o{s // 500}", "family": f"f{s // 60}", "genus": f"g{s // 4}", "species": f"s{s}"}


def make_split(n, species, centers, gen, dev, noise):
    import torch

    from clibd_amd import ops

    sp = species[torch.randint(0, len(species), (n,), generator=gen)]
    x = centers[sp.to(dev)] + noise * torch.randn(n, centers.shape[1], generator=gen).to(dev)
    return ops.l2norm_fwd(x.contiguous())[0], [taxonomy(int(s)) for s in sp.tolist()]


def reference_convention(splits, thresholds, k_list):
    """species top-1 hits [len(thresholds), n_splits] the way the reference gets them"""
    out = []
    for threshold in thresholds:
        row = []
        for pred_a, conf, pred_b, gt in splits:
            final = []
            for pa, cs, pb in zip(pred_a, conf, pred_b):
                cur = {}
                for kth in range(len(cs)):
                    src = pa if cs[kth] > threshold else pb
                    for level in src.keys():
                        cur.setdefault(level, []).append(src[level][kth])
                final.append(cur)
            micro = {}
            for k in k_list:
                micro[k] = {}
                for level in LEVELS:
                    correct = 0
                    for p, g in zip(final, gt):
                        if g[level] in p[level][:k]:
                            correct += 1
                    micro[k][level] = correct * 1.0 / len(final)
            row.append(micro[1]["species"])
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seen-keys", type=int, default=12000)
    ap.add_argument("--unseen-keys", type=int, default=9118)
    ap.add_argument("--seen", type=int, default=8000)
    ap.add_argument("--unseen", type=int, default=8000)
    ap.add_argument("--species", type=int, default=8000)
    ap.add_argument("--thresholds", type=int, default=1000)
    ap.add_argument("--cpu-thresholds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from clibd_amd import eval as E
    from clibd_amd import method_nn as M
    from clibd_amd import ops
    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    S = a.species
    centers = torch.randn(S, 768, generator=gen).to(dev)
    seen_sp, unseen_sp = torch.arange(S // 2), torch.arange(S // 2, S)
    seen_keys, seen_keys_label = make_split(a.seen_keys, seen_sp, centers, gen, dev, 1.5)
    unseen_keys, unseen_keys_label = make_split(a.unseen_keys, unseen_sp, centers, gen, dev, 1.2)
    seen_q, seen_gt = make_split(a.seen, seen_sp, centers, gen, dev, 1.5)
    unseen_q, unseen_gt = make_split(a.unseen, unseen_sp, centers, gen, dev, 1.5)
    grid = np.linspace(0, 1, a.thresholds)

    def whole(with_predictions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = M.seen_unseen_from_features(seen_q, unseen_q, seen_keys, seen_keys_label, unseen_keys, unseen_keys_label, seen_gt, unseen_gt, K_LIST,
                                          thresholds=grid, with_predictions=with_predictions)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    whole(True)                                                               # warm-up
    t_pred = min(whole(True)[0] for _ in range(a.reps))
    runs = [whole(False) for _ in range(a.reps)]
    t_idx, (seen_out, unseen_out) = min(r[0] for r in runs), runs[0][1]

    # ---- the threshold search alone, on the two finished searches
    m = 5
    queries = torch.cat([seen_q, unseen_q])
    conf, idx_a = E.topk_search(queries, E.prepare_key_bank(seen_keys), m, cache=False)
    _, idx_b = E.topk_search(queries, E.prepare_key_bank(unseen_keys), m, cache=False)
    codec = E.LabelCodec()
    ids_a, ids_b = codec.encode(seen_keys_label), codec.encode(unseen_keys_label)
    q_ids = torch.from_numpy(np.concatenate([codec.encode(seen_gt), codec.encode(unseen_gt)])).to(dev)
    table_a, table_b = torch.from_numpy(ids_a).to(dev), torch.from_numpy(ids_b).to(dev)
    segment = torch.from_numpy(np.repeat(np.array([0, 1], dtype=np.int32), [a.seen, a.unseen])).to(dev)
    thr_d = torch.from_numpy(grid).to(dev)

    def device_search():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hits = ops.threshold_sweep_hits(conf, idx_a, idx_b, table_a, table_b, q_ids, thr_d, [1], segment=segment, nseg=2).cpu().numpy()[:, :, 0, 3]
        best = M.choose_threshold(hits, [a.seen, a.unseen], grid)
        return time.perf_counter() - t0, hits, best

    device_search()
    t_dev, hits, best = min((device_search() for _ in range(a.reps)), key=lambda r: r[0])
    assert best == seen_out["best_threshold"]

    def kernels_only():                                                       # device time of the two sweep kernels, all k of K_LIST
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            ops.threshold_sweep_hits(conf, idx_a, idx_b, table_a, table_b, q_ids, thr_d, K_LIST, segment=segment, nseg=2)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 20

    t_kernels = kernels_only()

    # ---- the reference's convention on the CPU, on a stated subset of the thresholds
    conf_h, ia_h, ib_h = conf.cpu().numpy(), idx_a.cpu().numpy(), idx_b.cpu().numpy()
    splits = []
    for lo, hi, gt in ((0, a.seen, seen_gt), (a.seen, a.seen + a.unseen, unseen_gt)):
        splits.append((codec.decode_rows(ids_a, ia_h[lo:hi]), conf_h[lo:hi].tolist(), codec.decode_rows(ids_b, ib_h[lo:hi]), gt))
    sub = np.unique(np.linspace(0, a.thresholds - 1, a.cpu_thresholds).round().astype(int))
    t0 = time.perf_counter()
    acc = reference_convention(splits, grid[sub], K_LIST)
    t_cpu_sub = time.perf_counter() - t0
    for row, t in zip(acc, sub):
        assert row == [int(hits[t, 0]) * 1.0 / a.seen, int(hits[t, 1]) * 1.0 / a.unseen], "device counts and the reference convention disagree"
    t_cpu = t_cpu_sub * a.thresholds / len(sub)

    rec = {"tool": "bench_method_nn", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "seen_keys": a.seen_keys,
           "unseen_keys": a.unseen_keys, "seen": a.seen, "unseen": a.unseen, "species": S, "D": 768, "m": m, "thresholds": a.thresholds,
           "k_list": K_LIST, "threshold_search_device_ms": round(t_dev * 1e3, 3), "sweep_kernels_device_ms_all_k": round(t_kernels, 4),
           "threshold_search_reference_cpu_s_scaled": round(t_cpu, 2), "cpu_thresholds_timed": int(len(sub)),
           "cpu_seconds_measured": round(t_cpu_sub, 3), "seen_unseen_from_features_s_with_predictions": round(t_pred, 4),
           "seen_unseen_from_features_s_index_arrays": round(t_idx, 4), "best_threshold": float(best),
           "top1_species_seen": seen_out["micro_acc"][1]["species"], "top1_species_unseen": unseen_out["micro_acc"][1]["species"]}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
