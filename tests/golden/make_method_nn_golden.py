"""Generate tests/golden/method_nn_golden.pt: the reference's seen/unseen classification by similarity threshold (scripts/method_nn.py)
on synthetic features (authoring container only).

    python tests/golden/make_method_nn_golden.py       # needs /root/reference; writes tests/golden/method_nn_golden.pt

The reference's scripts/method_nn.py is imported with the stub pattern of make_golden.py / make_eval_golden.py: hydra.main a no-op
decorator, faiss.IndexFlatIP the exact float32 numpy search of make_eval_golden.py, get_feature_and_label replaced by the synthetic
features below (the five "dataloaders" are the names of the five splits).  Only data is written: integer hit counts, thresholds,
accuracy tables, predicted labels as small integer codes, the searches' indices and similarities, seeds, redraw counts and checksums.
The features themselves are regenerated from numpy's legacy RandomState by `synth`.

Unlike make_eval_golden.synth_split, the image and the DNA embedding of a species share ONE centre (image -> DNA retrieval would sit
at chance otherwise): image = centre + 1.5 noise, DNA = centre + 1.2 noise, unit rows.  Seen species: the first 60 %; the seen keys
miss the last two of them and the unseen keys the last two unseen ones, so some queries have a species no key has.

Two sets: "small" (600 seen keys: the exact search) and "large" (4 200 seen keys: the pre-filtered search).  Recorded per set:
  hits[n]           the reference's species top-1 hit counts [n, 2] (seen, unseen) per threshold of np.linspace(0, 1, n), n = 1000, 1001
                    (from its make_final_pred + top_k_micro_accuracy, acc * Q checked to be the integer)
  best[n]           the threshold its search_threshold_with_harmonic_mean chose on that grid
  out               the two output dicts of its method_1_inference_and_eval_for_seen_and_unseen (predictions as codes)
  out_at            the same from get_final_pred_and_acc at a given threshold (0.25), for `searched_threshold=`
  decide            decide_prediction_with_threshold of the seen split at three thresholds (codes)
  search            per split the seen-key search's similarities (fp32) and both searches' indices (the list convention's inputs)
The generator asserts what keeps the fixture from hiding a failure (see `make_set`): every top-m similarity of the seen-key search is
more than 1e-5 from every threshold of both grids and the top-(m + 1) scores of both searches are more than 1e-5 apart (offending
query rows are redrawn, the redraw recorded); the chosen threshold is interior, both accuracies at it are >= 0.3, the harmonic curve
takes >= 50 distinct values, >= 20 merged lists mix both sources, and in at least one set the maximum is attained at >= 2 thresholds.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
LEVELS = ["order", "family", "genus", "species"]
D = 128
K_LIST = [1, 3, 5]
M = 5                      # the reference searches with max_k = 5
GAP = 1e-5
GRIDS = (1000, 1001)
GIVEN_THRESHOLD = 0.25
DECIDE_AT = (0.2, 0.3337, 0.45)
SPLITS = ("seen_keys", "val_unseen_keys", "test_unseen_keys", "seen_query", "unseen_query")
SETS = {"small": dict(seed=31, n_seen_keys=600, n_val_keys=150, n_test_keys=150, n_seen=200, n_unseen=150, n_species=60),
        "large": dict(seed=47, n_seen_keys=4200, n_val_keys=400, n_test_keys=400, n_seen=200, n_unseen=150, n_species=300)}


def taxonomy(s: int) -> dict:
    return {"order": f"o{s // 27}", "family": f"f{s // 9}", "genus": f"g{s // 3}", "species": f"s{s}"}


def species_of(cfg) -> dict:
    rs = np.random.RandomState(cfg["seed"])
    S = cfg["n_species"]
    n_seen_sp = int(S * 0.6)
    return {"seen_keys": rs.randint(0, n_seen_sp - 2, cfg["n_seen_keys"]), "val_unseen_keys": rs.randint(n_seen_sp, S - 2, cfg["n_val_keys"]),
            "test_unseen_keys": rs.randint(n_seen_sp, S - 2, cfg["n_test_keys"]), "seen_query": rs.randint(0, n_seen_sp, cfg["n_seen"]),
            "unseen_query": rs.randint(n_seen_sp, S, cfg["n_unseen"])}


def synth(cfg, split: str, redraw=None):
    """(image, dna) fp32 [N, D] unit rows of one split around species centres shared by the two modalities"""
    sp = species_of(cfg)[split]
    centers = np.random.RandomState(cfg["seed"] + 1).randn(cfg["n_species"], D)
    sid = SPLITS.index(split)
    out = np.empty((2, len(sp), D), dtype=np.float32)
    noise = np.array([[1.5], [1.2]])
    for i, s in enumerate(sp):
        a = 0 if redraw is None else int(redraw[i])
        rs = np.random.RandomState([cfg["seed"], sid, i, a])
        x = centers[s][None, :] + noise * rs.randn(2, D)
        out[:, i] = (x / np.sqrt(np.sum(x * x, axis=1, keepdims=True))).astype(np.float32)
    return out[0], out[1]


def labels_of(sp):
    return [taxonomy(int(s)) for s in sp]


def checksum(feats) -> float:
    return float(sum(np.sum(f.astype(np.float64) * np.arange(1, f.size + 1).reshape(f.shape) % 1000.0) for f in feats))


def all_thresholds() -> np.ndarray:
    return np.unique(np.concatenate([np.linspace(0, 1, n) for n in GRIDS]))


def bad_rows(q_img, keys_a, keys_b) -> set:
    """query rows whose top-(M + 1) scores of either search are within GAP of each other, or whose top-M seen-key similarities are within
    GAP of a threshold of either grid"""
    grid = all_thresholds()
    bad = set()
    for n, keys in enumerate((keys_a, keys_b)):
        s = np.sort(q_img.astype(np.float32) @ keys.astype(np.float32).T, axis=1)[:, ::-1][:, : M + 1].astype(np.float64)
        bad |= set(np.nonzero((s[:, :-1] - s[:, 1:]).min(axis=1) <= GAP)[0].tolist())
        if n == 0:
            top = s[:, :M]
            pos = np.clip(np.searchsorted(grid, top), 1, len(grid) - 1)
            dist = np.minimum(np.abs(top - grid[pos - 1]), np.abs(top - grid[pos]))
            bad |= set(np.nonzero(dist.min(axis=1) <= GAP)[0].tolist())
    return bad


class Args:
    def __init__(self, k_list):
        self.inference_and_eval_setting = types.SimpleNamespace(k_list=k_list)


class _Model:
    def eval(self):
        return self


def import_reference():
    sys.path.insert(0, HERE)
    import make_eval_golden as EG
    import make_golden as MG

    MG.install_stubs()
    MG._stub("umap", UMAP=MG._Anything)
    MG._stub("hydra", main=lambda *a, **k: (lambda f: f))
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except Exception:
            MG._stub("tqdm", tqdm=lambda it, *a, **k: it)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "scripts"))
    import importlib.util

    import bioscanclip.util.util as U

    U.faiss.IndexFlatIP = EG.ExactIP
    spec = importlib.util.spec_from_file_location("ref_method_nn", os.path.join(REF, "scripts", "method_nn.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)

    class _Quiet:                       # the reference's progress bar, silenced
        def __init__(self, it, *a, **k):
            self.it = it

        def __iter__(self):
            return iter(self.it)

        def set_description(self, *a, **k):
            pass

    R.tqdm = _Quiet
    return U, R, EG


def encode_preds(pred_list, vocab):
    return np.array([[[vocab[l][x] for x in p[lv]] for l, lv in enumerate(LEVELS)] for p in pred_list], dtype=np.uint16)


def pack_out(out, vocab):
    return {"final_pred_codes": encode_preds(out["final_pred_labels"], vocab), "best_threshold": float(out["best_threshold"]),
            "micro_acc": out["micro_acc"], "macro_acc": out["macro_acc"], "per_class_acc": out["per_class_acc"]}


def make_set(U, R, EG, cfg):
    args = Args(K_LIST)
    sps = species_of(cfg)
    redraw = {"seen_query": np.zeros(cfg["n_seen"], np.int64), "unseen_query": np.zeros(cfg["n_unseen"], np.int64)}
    key_feats = {s: synth(cfg, s) for s in SPLITS[:3]}
    keys_a = key_feats["seen_keys"][0]
    keys_b = np.concatenate([key_feats["val_unseen_keys"][1], key_feats["test_unseen_keys"][1]])
    for _ in range(40):
        todo = {s: bad_rows(synth(cfg, s, redraw[s])[0], keys_a, keys_b) for s in redraw}
        if not any(todo.values()):
            break
        for s, rows in todo.items():
            for r in rows:
                redraw[s][r] += 1
    else:
        raise RuntimeError("score gaps / threshold distances not reached")
    feats = {s: synth(cfg, s, redraw.get(s)) for s in SPLITS}

    def fake_get_feature_and_label(dataloader, model, device, **kw):
        img, dna = feats[dataloader]
        return [f"{dataloader}{i}" for i in range(len(img))], img.astype(np.float64), dna.astype(np.float64), None, labels_of(sps[dataloader])

    R.get_feature_and_label = fake_get_feature_and_label
    S = cfg["n_species"]
    vocab = [{taxonomy(s)[lv]: None for s in range(S)} for lv in LEVELS]
    vocab = [{x: i for i, x in enumerate(v)} for v in vocab]

    # the reference end to end (its own grid of 1 000 thresholds)
    seen_out, unseen_out = R.method_1_inference_and_eval_for_seen_and_unseen(args, _Model(), "seen_query", "unseen_query", "seen_keys", "val_unseen_keys",
                                                                             "test_unseen_keys", "cpu")
    # its two searches once more, for the per-threshold counts and the list convention's inputs
    EG.ExactIP.calls = []
    sa, sim_s, gt_s, ua, sim_u, gt_u = R.inference_with_original_image_encoder_and_dna_encoder(_Model(), "seen_query", "unseen_query", ["seen_keys"], "cpu",
                                                                                               key_type="image")
    sb, _, _, ub, _, _ = R.inference_with_original_image_encoder_and_dna_encoder(_Model(), "seen_query", "unseen_query",
                                                                                 ["val_unseen_keys", "test_unseen_keys"], "cpu", key_type="dna")
    idx_sa, idx_ua, idx_sb, idx_ub = EG.ExactIP.calls
    splits = [{"pred_labels_from_search_with_seen_keys": sa, "pred_labels_from_search_with_unseen_keys": sb,
               "pred_similarity_from_search_with_seen_keys": sim_s.tolist(), "gt_label": gt_s},
              {"pred_labels_from_search_with_seen_keys": ua, "pred_labels_from_search_with_unseen_keys": ub,
               "pred_similarity_from_search_with_seen_keys": sim_u.tolist(), "gt_label": gt_u}]
    grid_all = all_thresholds()
    for sim in (sim_s, sim_u):          # the reference's own similarities keep the distance too
        assert np.abs(sim.astype(np.float64)[:, :, None] - grid_all[None, None, :]).min() > GAP
    hits, best, curves = {}, {}, {}
    for n in GRIDS:
        h = np.zeros((n, 2), dtype=np.int32)
        for t, thr in enumerate(np.linspace(0, 1, n)):
            for s, sp in enumerate(splits):
                final, gt = R.make_final_pred(args, sp["pred_labels_from_search_with_seen_keys"], sp["pred_similarity_from_search_with_seen_keys"],
                                              sp["pred_labels_from_search_with_unseen_keys"], sp["gt_label"], threshold=thr)
                acc = R.top_k_micro_accuracy(final, gt, k_list=K_LIST)[1]["species"]
                h[t, s] = int(round(acc * len(gt)))
                assert h[t, s] * 1.0 / len(gt) == acc
        hits[n] = h
        best[n] = float(R.search_threshold_with_harmonic_mean(args, splits, num_intervals=n))
        curves[n] = np.array([R.harmonic_mean([h[t, 0] * 1.0 / len(gt_s), h[t, 1] * 1.0 / len(gt_u)]) for t in range(n)])
    assert best[1000] == float(seen_out["best_threshold"]) == float(unseen_out["best_threshold"])

    # ---- the fixture must not hide a failure
    plateau = {}
    for n in GRIDS:
        grid, c = np.linspace(0, 1, n), curves[n]
        t = int(np.nonzero(grid == best[n])[0][0])
        assert 0 < t < n - 1, "the chosen threshold is the first or the last grid point"
        assert t == int(np.argmax(c)) and hits[n][t, 0] / len(gt_s) >= 0.3 and hits[n][t, 1] / len(gt_u) >= 0.3
        assert len(np.unique(c)) >= 50
        plateau[n] = int((c == c.max()).sum())
    mixed = 0
    for sim in (sim_s, sim_u):
        sel = (sim.astype(np.float64) > best[1000]).sum(axis=1)
        mixed += int(((sel > 0) & (sel < M)).sum())
    assert mixed >= 20, mixed

    at = [R.get_final_pred_and_acc(args, sp["pred_labels_from_search_with_seen_keys"], sp["pred_similarity_from_search_with_seen_keys"],
                                   sp["pred_labels_from_search_with_unseen_keys"], sp["gt_label"], best_threshold=GIVEN_THRESHOLD) for sp in splits]
    decide = {thr: encode_preds(R.decide_prediction_with_threshold(args, sa, sim_s.tolist(), sb, thr), vocab) for thr in DECIDE_AT}
    return {"cfg": cfg, "redraw": {s: r.copy() for s, r in redraw.items()}, "checksum": {s: checksum(f) for s, f in feats.items()},
            "species": {s: v.astype(np.int16) for s, v in sps.items()}, "k_list": K_LIST, "vocab": [list(v) for v in vocab],
            "hits": hits, "best": best, "plateau": plateau, "mixed": mixed,
            "out": {"seen": pack_out(seen_out, vocab), "unseen": pack_out(unseen_out, vocab)},
            "given_threshold": GIVEN_THRESHOLD, "out_at": {"seen": pack_out(at[0], vocab), "unseen": pack_out(at[1], vocab)},
            "decide": decide,
            "search": {"seen": {"sim_a": sim_s.astype(np.float32), "idx_a": idx_sa.astype(np.int16), "idx_b": idx_sb.astype(np.int16)},
                       "unseen": {"sim_a": sim_u.astype(np.float32), "idx_a": idx_ua.astype(np.int16), "idx_b": idx_ub.astype(np.int16)}}}


def main():
    import torch

    U, R, EG = import_reference()
    out = {name: make_set(U, R, EG, cfg) for name, cfg in SETS.items()}
    assert max(max(out[n]["plateau"].values()) for n in SETS) >= 2, "no set exercises the first-maximum rule"
    path = os.path.join(HERE, "method_nn_golden.pt")
    torch.save(out, path)
    for n in SETS:
        g = out[n]
        print(f"{n}: best {g['best']}, plateau {g['plateau']}, mixed {g['mixed']}, redrawn rows "
              f"{int(sum((r > 0).sum() for r in g['redraw'].values()))}, top-1 at best "
              f"{g['out']['seen']['micro_acc'][1]['species']:.3f} / {g['out']['unseen']['micro_acc'][1]['species']:.3f}")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
