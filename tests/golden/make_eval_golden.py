"""Generate tests/golden/eval_golden.pt: the reference's eval-phase accuracy tables on synthetic features (authoring container only).

    python tests/golden/make_eval_golden.py       # needs /root/reference; writes tests/golden/eval_golden.pt

The features are not stored: `synth_split` regenerates them from numpy's legacy RandomState (a frozen stream) and the golden
records a checksum of every split.  The reference (bioscanclip.util.util, scripts/train_cl.py) is imported with the stub pattern of
make_golden.py; faiss.IndexFlatIP becomes the exact float32 numpy search below and print_micro_and_macro_acc a no-op.  Only data
is written: labels as small integer codes, the reference's acc_dict / per_class_acc, its predicted labels as codes, and the
indices its searches returned.

Two sets: "small" (600 keys, 200 seen + 150 unseen queries, D = 128: the exact search) and "large" (4 200 keys: every key type
takes the pre-filtered search).  Queries include species absent from the keys and many keys share a species.  Every search's
top-(max_k + 1) scores are separated by more than 1e-5 (a query row failing that is redrawn, the redraw recorded), so the index
lists cannot depend on fp32 vs float64 arithmetic.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
LEVELS = ["order", "family", "genus", "species"]
D = 128
K_LIST = [1, 3, 5]
GAP = 1e-5
SETS = {"small": dict(seed=11, n_keys=600, n_seen=200, n_unseen=150, n_species=60),
        "large": dict(seed=23, n_keys=4200, n_seen=200, n_unseen=150, n_species=90)}


def taxonomy(s: int) -> dict:
    """species s -> its four labels (strings, as BIOSCAN's): 3 species per genus, 3 genera per family, 3 families per order"""
    return {"order": f"o{s // 27}", "family": f"f{s // 9}", "genus": f"g{s // 3}", "species": f"s{s}"}


def species_of(cfg):
    """(key, seen, unseen) species ids.  Seen species: the first 60 %; unseen: the rest, of which the last 4 never occur among the keys."""
    rs = np.random.RandomState(cfg["seed"])
    S = cfg["n_species"]
    n_seen_sp = int(S * 0.6)
    key_sp = rs.randint(0, S - 4, cfg["n_keys"])
    seen_sp = rs.randint(0, n_seen_sp, cfg["n_seen"])
    unseen_sp = rs.randint(n_seen_sp, S, cfg["n_unseen"])
    return key_sp, seen_sp, unseen_sp


def synth_split(cfg, split: str, redraw=None):
    """(image, dna, text) fp32 [N, D] unit rows, clustered by species, of split 'keys' / 'seen' / 'unseen'; redraw[i] = how often row i was redrawn"""
    key_sp, seen_sp, unseen_sp = species_of(cfg)
    sp = {"keys": key_sp, "seen": seen_sp, "unseen": unseen_sp}[split]
    centers = np.random.RandomState(cfg["seed"] + 1).randn(3, cfg["n_species"], D)
    sid = {"keys": 0, "seen": 1, "unseen": 2}[split]
    out = np.empty((3, len(sp), D), dtype=np.float32)
    for i, s in enumerate(sp):
        a = 0 if redraw is None else int(redraw[i])
        rs = np.random.RandomState([cfg["seed"], sid, i, a])
        x = centers[:, s] + 0.7 * rs.randn(3, D)
        out[:, i] = (x / np.sqrt(np.sum(x * x, axis=1, keepdims=True))).astype(np.float32)
    return out[0], out[1], out[2]


def labels_of(sp):
    return [taxonomy(int(s)) for s in sp]


def checksum(feats) -> float:
    return float(sum(np.sum(f.astype(np.float64) * np.arange(1, f.size + 1).reshape(f.shape) % 1000.0) for f in feats))


class ExactIP:
    """faiss.IndexFlatIP stand-in: exact float32 inner products, top-k by (score descending, index ascending)."""
    calls = []

    def __init__(self, d):
        self.keys = np.zeros((0, d), dtype=np.float32)

    def add(self, x):
        self.keys = np.concatenate([self.keys, np.asarray(x, dtype=np.float32)])

    def search(self, q, k):
        s = np.asarray(q, dtype=np.float32) @ self.keys.T
        idx = np.argsort(-s, axis=1, kind="stable")[:, :k]
        ExactIP.calls.append(idx.copy())
        return np.take_along_axis(s, idx, 1), idx


def import_reference():
    sys.path.insert(0, HERE)
    import make_golden as M

    M.install_stubs()
    M._stub("umap", UMAP=M._Anything)
    M._stub("hydra", main=lambda *a, **k: (lambda f: f))
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "scripts"))
    import importlib.util

    import bioscanclip.util.util as U

    spec = importlib.util.spec_from_file_location("train_cl", os.path.join(REF, "scripts", "train_cl.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    U.faiss.IndexFlatIP = ExactIP
    U.print_micro_and_macro_acc = lambda *a, **k: None
    return U, T


def ref_dicts(U, cfg, redraw):
    """the reference's get_features_and_label dictionaries, its embedding loop replaced by the synthetic float64 features"""
    out = {}
    sps = dict(zip(("keys", "seen", "unseen"), species_of(cfg)))
    for split in ("keys", "seen", "unseen"):
        img, dna, txt = (f.astype(np.float64) for f in synth_split(cfg, split, redraw.get(split)))
        labels = labels_of(sps[split])
        U.get_feature_and_label = lambda *a, **k: ([f"{split}{i}" for i in range(len(labels))], img, dna, txt, labels)
        out[split] = U.get_features_and_label(None, _Model(), "cpu", for_key_set=(split == "keys"))
    return out


class _Model:
    def eval(self):
        return self


def gaps_ok(keys_dict, q_dict, max_k):
    """rows of q_dict whose top-(max_k + 1) scores against some matching key type are closer than GAP"""
    bad = set()
    for qt in ("encoded_image_feature", "encoded_dna_feature", "encoded_language_feature", "averaged_feature", "concatenated_feature"):
        for kt in ("encoded_image_feature", "encoded_dna_feature", "encoded_language_feature", "averaged_feature", "concatenated_feature", "all_key_features"):
            q, k = q_dict[qt], keys_dict[kt]
            if q.shape[1] != k.shape[1]:
                continue
            qn = q / np.linalg.norm(q, axis=1, keepdims=True)
            kn = k / np.linalg.norm(k, axis=1, keepdims=True)
            s = np.sort(qn @ kn.T, axis=1)[:, ::-1][:, : max_k + 1]
            bad |= set(np.nonzero((s[:, :-1] - s[:, 1:]).min(axis=1) <= GAP)[0].tolist())
    return bad


def encode_preds(pred_list, vocab):
    return np.array([[[vocab[l][x] for x in p[lv]] for l, lv in enumerate(LEVELS)] for p in pred_list], dtype=np.uint8)


def make_set(U, T, cfg):
    redraw = {"seen": np.zeros(cfg["n_seen"], np.int64), "unseen": np.zeros(cfg["n_unseen"], np.int64)}
    for _ in range(40):
        d = ref_dicts(U, cfg, redraw)
        todo = {s: gaps_ok(d["keys"], d[s], K_LIST[-1]) for s in ("seen", "unseen")}
        if not any(todo.values()):
            break
        for s, rows in todo.items():
            for r in rows:
                redraw[s][r] += 1
    else:
        raise RuntimeError("score gaps not reached")
    ExactIP.calls = []
    acc, per_class, pred = U.inference_and_print_result(d["keys"], d["seen"], d["unseen"], None, k_list=K_LIST)
    overall = T.compute_overall_acc(acc)
    S = cfg["n_species"]
    vocab = [{taxonomy(s)[lv]: None for s in range(S)} for lv in LEVELS]
    vocab = [{x: i for i, x in enumerate(v)} for v in vocab]
    codes, idx = {}, {}
    calls = iter(ExactIP.calls)
    for qt, per_key in pred.items():
        if qt.endswith("_id") or qt.endswith("_gt_label"):
            continue
        for kt, pr in per_key.items():
            if not pr:
                continue
            codes[(qt, kt)] = (encode_preds(pr["curr_seen_pred_list"], vocab), encode_preds(pr["curr_unseen_pred_list"], vocab))
            idx[(qt, kt)] = (next(calls).astype(np.int16), next(calls).astype(np.int16))
    sps = species_of(cfg)
    feats = {s: synth_split(cfg, s, redraw.get(s)) for s in ("keys", "seen", "unseen")}
    # the reference's own dict construction on the small set's first rows (averaged / concatenated / all_key_features)
    construct = {kk: (v[:5].astype(np.float32) if isinstance(v, np.ndarray) else v[:5]) for kk, v in d["keys"].items() if v is not None}
    return {"cfg": cfg, "redraw": {s: r.copy() for s, r in redraw.items()}, "checksum": {s: checksum(f) for s, f in feats.items()},
            "species": dict(zip(("keys", "seen", "unseen"), [s.astype(np.int16) for s in sps])), "k_list": K_LIST,
            "acc_dict": acc, "per_class_acc": per_class, "overall_acc": overall, "pred_codes": codes, "pred_idx": idx,
            "vocab": [list(v) for v in vocab], "construct_head": construct,
            "all_key_rows": int(d["keys"]["all_key_features"].shape[0])}


def make_standalone(U):
    """top_k_micro/macro_accuracy on random prediction lists with heavy label ties: 4 labels per level, lists of 8 with repeats"""
    rs = np.random.RandomState(5)
    Q = 300
    gt = rs.randint(0, 4, (Q, 4)).astype(np.int8)
    preds = rs.randint(0, 4, (Q, 4, 8)).astype(np.int8)
    gt_l = [{lv: f"{lv[0]}{gt[q, l]}" for l, lv in enumerate(LEVELS)} for q in range(Q)]
    pr_l = [{lv: [f"{lv[0]}{x}" for x in preds[q, l]] for l, lv in enumerate(LEVELS)} for q in range(Q)]
    ks = [1, 2, 4, 8]
    micro = U.top_k_micro_accuracy(pr_l, gt_l, k_list=ks)
    macro, per_class = U.top_k_macro_accuracy(pr_l, gt_l, k_list=ks)
    return {"gt": gt, "preds": preds, "k_list": ks, "micro": micro, "macro": macro, "per_class": per_class}


def main():
    import torch

    U, T = import_reference()
    out = {name: make_set(U, T, cfg) for name, cfg in SETS.items()}
    out["standalone"] = make_standalone(U)
    path = os.path.join(HERE, "eval_golden.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes); redrawn rows: "
          + ", ".join(f"{n} {int((out[n]['redraw']['seen'] > 0).sum() + (out[n]['redraw']['unseen'] > 0).sum())}" for n in SETS))


if __name__ == "__main__":
    main()
