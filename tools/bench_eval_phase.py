"""End-to-end time of the eval phase's scoring step (clibd_amd.eval.inference_and_print_result) at BIOSCAN-1M's shape.

    python tools/bench_eval_phase.py [--keys 21118] [--seen 8000] [--unseen 8000] [--reps 3] [--out profiles/eval_phase.log]

Synthetic features: image, DNA and text embeddings (D = 768) clustered by species (8 000 species in a 4-level hierarchy; the last 200
species occur only among the unseen queries), so the key types include averaged, concatenated and all_key_features (63 354 keys).
After one warm-up call it times
  1. inference_and_print_result with with_predictions=True (label lists in pred_dict, as the reference) and False (index arrays);
  2. the accuracy step alone for one search (image -> image, seen queries): the device counts (clibd_topk_label_hits + the host
     finaliser) against the reference's convention on the CPU (per-query Python label lists and `gt in pred[:k]` loops, restated here).
Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = ["order", "family", "genus", "species"]


def taxonomy(s: int) -> dict:
    return {"order": f"o{s // 500}", "family": f"f{s // 60}", "genus": f"g{s // 4}", "species": f"s{s}"}


def make_split(n, species, centers, gen, dev, noise=1.2):
    import torch

    from clibd_amd import ops

    sp = species[torch.randint(0, len(species), (n,), generator=gen)]
    feats = []
    for m in range(3):
        x = centers[m][sp.to(dev)] + noise * torch.randn(n, centers.shape[2], generator=gen).to(dev)
        feats.append(ops.l2norm_fwd(x.contiguous())[0])
    avg, cat = ops.eval_pair_features(feats[0], feats[1])
    labels = [taxonomy(int(s)) for s in sp.tolist()]
    return {"file_name_list": [f"q{i}" for i in range(n)], "encoded_image_feature": feats[0], "encoded_dna_feature": feats[1],
            "encoded_language_feature": feats[2], "averaged_feature": avg, "concatenated_feature": cat, "label_list": labels,
            "all_key_features": None, "all_key_features_label": None}


def reference_convention(pred_list, gt_list, k_list):
    """top_k_micro_accuracy + top_k_macro_accuracy as the reference computes them: Python loops over label lists"""
    micro, macro = {}, {}
    for k in k_list:
        micro[k], macro[k] = {}, {}
        for level in LEVELS:
            hit, cnt, correct = {}, {}, 0
            for p, g in zip(pred_list, gt_list):
                lab = g[level]
                ok = lab in p[level][:k]
                correct += ok
                hit[lab] = hit.get(lab, 0) + ok
                cnt[lab] = cnt.get(lab, 0) + 1
            micro[k][level] = correct * 1.0 / len(pred_list)
            s = 0
            for lab in cnt:
                s = s + hit[lab] * 1.0 / cnt[lab]
            macro[k][level] = s / len(cnt)
    return micro, macro


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=21118)
    ap.add_argument("--seen", type=int, default=8000)
    ap.add_argument("--unseen", type=int, default=8000)
    ap.add_argument("--species", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from clibd_amd import eval as E
    from clibd_amd import ops
    from clibd_amd.build import csrc_hash

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    S = a.species
    centers = torch.randn(3, S, 768, generator=gen).to(dev)
    keys = make_split(a.keys, torch.arange(S - 200), centers, gen, dev)
    keys["all_key_features"] = torch.cat([keys["encoded_image_feature"], keys["encoded_dna_feature"], keys["encoded_language_feature"]])
    keys["all_key_features_label"] = keys["label_list"] * 3
    seen = make_split(a.seen, torch.arange((S - 200) // 2), centers, gen, dev)
    unseen = make_split(a.unseen, torch.arange((S - 200) // 2, S), centers, gen, dev)
    k_list = [1, 3, 5]

    def run(with_predictions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            acc, _, _ = E.inference_and_print_result(keys, seen, unseen, k_list=k_list, with_predictions=with_predictions)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, acc

    run(True)                                                                 # warm-up (label codecs, kernels)
    t_pred = min(run(True)[0] for _ in range(a.reps))
    times = [run(False) for _ in range(a.reps)]
    t_idx, acc = min(t for t, _ in times), times[0][1]

    # ---- the accuracy step alone: image -> image, seen queries
    _, idx = E.topk_search(seen["encoded_image_feature"], keys["encoded_image_feature"], 5)
    codec, key_ids = E._cached_key_label_ids(keys["label_list"], dev)
    q_ids_h = codec.encode(seen["label_list"])
    q_ids = torch.from_numpy(q_ids_h).to(dev)

    def device_acc():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        off = codec.class_offset()
        _, lh, ch, cc = ops.topk_label_hits(idx, key_ids, q_ids, off, k_list)
        out = E._split_accuracy(lh.cpu().numpy()[0], ch.cpu().numpy()[0], cc.cpu().numpy()[0], q_ids_h, codec, off, k_list, [0, 1, 2])
        return time.perf_counter() - t0, out

    device_acc()
    t_dev, (micro_d, macro_d, _) = min((device_acc() for _ in range(a.reps)), key=lambda r: r[0])
    pred_list = codec.decode_rows(key_ids.cpu().numpy(), idx.cpu().numpy())
    t0 = time.perf_counter()
    micro_c, macro_c = reference_convention(pred_list, seen["label_list"], k_list)
    t_cpu = time.perf_counter() - t0
    assert micro_c == micro_d and macro_c == macro_d, "device counts and the reference convention disagree"

    n_searches = sum(1 for per_key in acc.values() for v in per_key.values() if v)
    rec = {"tool": "bench_eval_phase", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "keys": a.keys, "seen": a.seen,
           "unseen": a.unseen, "species": S, "D": 768, "k_list": k_list, "searches": n_searches,
           "inference_s_with_predictions": round(t_pred, 4), "inference_s_index_arrays": round(t_idx, 4),
           "accuracy_step_device_ms": round(t_dev * 1e3, 3), "accuracy_step_reference_cpu_ms": round(t_cpu * 1e3, 3),
           "top1_species_micro_seen_image_image": acc["encoded_image_feature"]["encoded_image_feature"]["seen"]["micro_acc"][1]["species"]}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
