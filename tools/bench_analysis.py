"""Time of the embedding analysis (clibd_amd.analysis) at BIOSCAN-1M's key-set shape.

    python tools/bench_analysis.py [--keys 21118] [--dim 768] [--seen 8000] [--unseen 8000] [--host-rows 4000] [--reps 3]
                                   [--out profiles/analysis.log]

N = 21 118 keys, D = 768, cluster sizes like BIOSCAN's: one order with 80 % of the rows, about N / 3 species.  After a warm-up it times
  1. the four-level silhouette (`silhouette_by_level`: sort, gather, clibd_silhouette_samples per level), wall clock, best of --reps, and
     the kernel alone per level as device-event time, next to the f32-MFMA roofline of its distance product (2 N^2 D FLOP at 155 TF);
  2. the nine-pair nearest same-species pass (clibd_same_label_nearest, 16 k queries) as device-event time;
  3. the confusion pass (clibd_confusion_counts at species level) as device-event time.
The host baseline is sklearn's silhouette_samples on the first --host-rows keys (its cost grows with N^2; the full set takes minutes) when
sklearn is present, otherwise the record says so.  Records, not gates: there is no parent to compare with.
Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MFMA_TFLOPS = 155.0


def device_ms(fn, iters=3, windows=3):
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
    ap.add_argument("--keys", type=int, default=21118)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--seen", type=int, default=8000)
    ap.add_argument("--unseen", type=int, default=8000)
    ap.add_argument("--host-rows", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from clibd_amd import analysis as A
    from clibd_amd import ops
    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    N, D = a.keys, a.dim
    S = max(N // 3, 8)
    # species sizes ~ a long tail; 80 % of the species (and so about 80 % of the rows) in order o0
    species = np.minimum((rs.pareto(1.5, N) * S / 8).astype(np.int64), S - 1)
    species[:S] = np.arange(S)
    order_of = np.where(np.arange(S) < 0.8 * S, 0, 1 + np.arange(S) % 15)
    labels = [{"order": f"o{order_of[s]}", "family": f"f{s // 60}", "genus": f"g{s // 4}", "species": f"s{s}"} for s in species.tolist()]
    gen = torch.Generator().manual_seed(0)
    centres = torch.randn(S, D, generator=gen).to(dev)
    sp_d = torch.from_numpy(species).to(dev)

    def feats(idx, noise):
        x = centres[idx] + noise * torch.randn(len(idx), D, generator=gen).to(dev)
        return ops.l2norm_fwd(x.contiguous())[0]

    keys = feats(sp_d, 1.2)

    # ---- 1. silhouette
    def four_levels():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = A.silhouette_by_level(keys, labels)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    four_levels()
    runs = [four_levels() for _ in range(a.reps)]
    t_four = min(r[0] for r in runs)
    means = {lv: float(s.double().mean()) for lv, s in runs[0][1].items()}
    codes = A.LabelCodec().encode(labels)
    kernel_ms, clusters = {}, {}
    for l, lv in enumerate(A.LEVELS):
        order, seg = A.plan_clusters(codes[:, l])
        xs = keys.index_select(0, torch.from_numpy(order).to(dev)).contiguous()
        ops.silhouette_samples(xs, seg)
        kernel_ms[lv] = round(device_ms(lambda: ops.silhouette_samples(xs, seg)), 3)
        clusters[lv] = len(seg) - 1
    flop = 2.0 * N * N * D
    roof_ms = flop / (F32_MFMA_TFLOPS * 1e12) * 1e3

    # ---- 2. nearest same-species key, nine pairs
    q_sp = torch.from_numpy(rs.randint(0, S, a.seen + a.unseen)).to(dev)
    mods_q = [feats(q_sp, n) for n in (1.5, 1.2, 0.5)]
    mods_k = [keys, feats(sp_d, 1.0), feats(sp_d, 0.4)]
    groups = A._Groups([d["species"] for d in labels], dev)
    qclass = torch.from_numpy(groups.query_classes([f"s{s}" for s in q_sp.tolist()])).to(dev)

    def nine():
        for q in mods_q:
            for k in mods_k:
                groups.nearest(q, k, qclass)

    nine()
    t_nine = device_ms(nine)

    # ---- 3. confusion at species level
    t_code = torch.from_numpy(rs.randint(0, S, a.seen + a.unseen).astype(np.int32)).to(dev)
    p_code = torch.from_numpy(rs.randint(-1, S, a.seen + a.unseen).astype(np.int32)).to(dev)
    ops.confusion_counts(t_code, p_code, S)
    t_conf = device_ms(lambda: ops.confusion_counts(t_code, p_code, S))

    # ---- host baseline
    host = {"host_baseline": "sklearn not present"}
    try:
        from sklearn.metrics import silhouette_samples

        n = min(a.host_rows, N)
        xh, ch = keys[:n].cpu().numpy(), codes[:n]
        t0 = time.perf_counter()
        for l in range(4):
            if 1 < len(np.unique(ch[:, l])) < n:
                silhouette_samples(xh, ch[:, l])
        t_host = time.perf_counter() - t0
        host = {"host_baseline": "sklearn.metrics.silhouette_samples, four levels", "host_rows": n, "host_s": round(t_host, 3),
                "host_s_scaled_to_keys": round(t_host * (N / n) ** 2, 1)}
    except ImportError:
        pass

    rec = {"tool": "bench_analysis", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "keys": N, "D": D, "clusters": clusters,
           "silhouette_four_levels_wall_s": round(t_four, 4), "silhouette_kernel_device_ms": kernel_ms,
           "distance_product_tflop_per_level": round(flop / 1e12, 3), "f32_mfma_roofline_ms_per_level": round(roof_ms, 3),
           "silhouette_tflops": {lv: round(flop / (ms * 1e-3) / 1e12, 1) for lv, ms in kernel_ms.items()}, "silhouette_means": means,
           "queries": a.seen + a.unseen, "nearest_nine_pairs_device_ms": round(t_nine, 3), "confusion_counts_device_ms": round(t_conf, 4),
           "confusion_classes": S, **host}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
