"""Generate tests/golden/method_linear_golden.pt: the reference's seen/unseen classification by a linear-probe classifier
(scripts/method_linear.py) on synthetic features (authoring container only).

    python tests/golden/make_method_linear_golden.py       # needs /root/reference; writes tests/golden/method_linear_golden.pt

The reference's scripts/method_linear.py is imported with the stub pattern of make_method_nn_golden.py: hydra and wandb no-ops,
faiss.IndexFlatIP the exact float32 numpy search of make_eval_golden.py, get_feature_and_label replaced by the synthetic features
below.  Only data is written: losses, the head before and after training, accuracy tables, fp32 confidences, class indices, integer
hit counts, thresholds, predicted labels as small integer codes, fp64 kernel references, seeds and redraw counts.  The features
themselves are regenerated from numpy's legacy RandomState by `synth` (tests import this module for it).

The synthetic world is make_method_nn_golden's: D = 128, 60 species around centres shared by the image and the DNA embedding (image =
centre + 1.5 noise, DNA = centre + 1.2 noise, unit rows); the first 36 species are the seen classes.  200 seen and 150 unseen
queries, 150 + 150 DNA keys of the unseen species, and a training set of 36 x 3 image features in batches of 48.

The reference's own ViTWIthExtraLayer(nn.Identity(), nn.Linear(128, 36)) is trained by its own fine_tuning_epoch with torch's AdamW
and OneCycleLR (LR / EPOCHS below: chosen so that the conditions at the end hold).  Recorded:
  head0 / head        the head before and after training (weight [36, 128], bias [36])
  step_losses         every step's loss.item(), epoch after epoch; epoch_losses, evaluation (evaluate_epoch's dict per epoch)
  conf / idx          per split the fp32 confidences and class indices of inference_with_fine_tuned_image_encoder
  idx_b               per split the image -> DNA search's indices
  hits                the reference's species top-1 hit counts [1001, 2] per threshold of np.linspace(0, 1, 1001)
  best                the threshold its search_threshold_with_harmonic_mean chose
  out / out_at        the two output dicts of its method_2_inference_and_eval_for_seen_and_unseen at the searched threshold and at a
                      given one (predictions as codes)
  kernel              at (B, C, D) = (33, 36, 128) — the first 33 seen queries, the trained head, their classes — fp64 logits, loss
                      (mean cross-entropy), dx, dw, db
The generator asserts what keeps the fixture from hiding a failure.  GAP = 2e-5, about six times the confidence error a CPU emulation
of the split-bf16 head showed (2.7e-6 .. 3.5e-6).  A query row is redrawn (the redraw recorded) while: one of its top-5 confidences
lies within GAP of an interior threshold or is not strictly positive; two neighbouring values of its top-6 probabilities lie within
GAP of each other; two neighbouring values of its top-6 DNA-search scores lie within 1e-5 of each other.  And: the chosen threshold is
interior, both accuracies at it are >= 0.3, the harmonic curve takes >= 50 distinct values, >= 20 merged lists mix both sources, the
median top-1 confidence lies between 0.3 and 0.9.
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
M = 5                      # the reference's torch.topk(..., k=5) and make_prediction(max_k=5)
GAP = 2e-5
SEARCH_GAP = 1e-5
NUM_INTERVALS = 1000       # the reference's grid: np.linspace(0, 1, NUM_INTERVALS + 1)
GIVEN_THRESHOLD = 0.25
SPLITS = ("train_seen", "val_unseen_keys", "test_unseen_keys", "seen_query", "unseen_query")
CFG = dict(seed=59, n_species=60, n_seen_species=36, n_train=36 * 3, n_val_keys=150, n_test_keys=150, n_seen=200, n_unseen=150)
BATCH = 36                 # training batch; the query loaders use QUERY_BATCH
QUERY_BATCH = 64
LR = 0.2                   # AdamW's lr and OneCycleLR's max_lr (the reference's main uses 1e-4 for both, on a real encoder)
EPOCHS = 24
HEAD_SEED = 7
KERNEL_ROWS = 33


def taxonomy(s: int) -> dict:
    return {"order": f"o{s // 27}", "family": f"f{s // 9}", "genus": f"g{s // 3}", "species": f"s{s}"}


def species_of(cfg=CFG) -> dict:
    rs = np.random.RandomState(cfg["seed"])
    S, C = cfg["n_species"], cfg["n_seen_species"]
    train = np.arange(cfg["n_train"]) % C          # every class appears
    rs.shuffle(train)
    return {"train_seen": train, "val_unseen_keys": rs.randint(C, S - 2, cfg["n_val_keys"]),
            "test_unseen_keys": rs.randint(C, S - 2, cfg["n_test_keys"]), "seen_query": rs.randint(0, C, cfg["n_seen"]),
            "unseen_query": rs.randint(C, S, cfg["n_unseen"])}


def synth(split: str, redraw=None, cfg=CFG):
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


def label_batch_of(sp) -> dict:
    return {lv: [taxonomy(int(s))[lv] for s in sp] for lv in LEVELS}


class Loader(list):
    """a list of the reference's 7-tuples (file names, image, dna, input_ids, token_type_ids, attention_mask, label dict) with a name;
    `image` holds the split's image FEATURES (the classifier's encoder is the identity)"""

    def __init__(self, name, batches):
        super().__init__(batches)
        self.name = name


def loader_of(split: str, feats: np.ndarray, batch: int, to_tensor):
    sp = species_of()[split]
    out = []
    for b0 in range(0, len(sp), batch):
        rows = slice(b0, b0 + batch)
        out.append(([f"{split}{i}" for i in range(b0, min(b0 + batch, len(sp)))], to_tensor(feats[rows]), None, None, None, None, label_batch_of(sp[rows])))
    return Loader(split, out)


def head0():
    """the head before training: nn.Linear(128, 36) under torch.manual_seed(HEAD_SEED) (recorded in the fixture as well)"""
    import torch

    torch.manual_seed(HEAD_SEED)
    lin = torch.nn.Linear(D, CFG["n_seen_species"])
    return lin


def fp64_case(x, w, b, t):
    """fp64 logits, mean cross-entropy, dx, dw, db of the head + CE at upstream gradient 1"""
    x, w, b = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    logits = x @ w.T + b
    mx = logits.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(logits - mx).sum(axis=1))
    B = x.shape[0]
    loss = float(np.mean(lse - logits[np.arange(B), t]))
    g = np.exp(logits - lse[:, None])
    g[np.arange(B), t] -= 1.0
    g /= B
    return {"logits": logits, "loss": loss, "dx": g @ w, "dw": g.T @ x, "db": g.sum(axis=0)}


def interior_grid() -> np.ndarray:
    return np.linspace(0, 1, NUM_INTERVALS + 1)[1:-1]


def bad_rows(q_img, w, b, keys_b) -> set:
    import torch
    import torch.nn.functional as F

    bad = set()
    with torch.no_grad():
        logits = F.linear(torch.from_numpy(q_img), torch.from_numpy(w), torch.from_numpy(b))
        p32 = F.softmax(logits, dim=-1).numpy()
    p = np.sort(p32.astype(np.float64), axis=1)[:, ::-1][:, : M + 1]
    bad |= set(np.nonzero((p[:, :-1] - p[:, 1:]).min(axis=1) <= GAP)[0].tolist())
    top = p[:, :M]
    bad |= set(np.nonzero((top <= 0).any(axis=1) | (top > 1).any(axis=1))[0].tolist())
    grid = interior_grid()
    pos = np.clip(np.searchsorted(grid, top), 1, len(grid) - 1)
    dist = np.minimum(np.abs(top - grid[pos - 1]), np.abs(top - grid[pos]))
    bad |= set(np.nonzero(dist.min(axis=1) <= GAP)[0].tolist())
    s = np.sort(q_img.astype(np.float32) @ keys_b.astype(np.float32).T, axis=1)[:, ::-1][:, : M + 1].astype(np.float64)
    bad |= set(np.nonzero((s[:, :-1] - s[:, 1:]).min(axis=1) <= SEARCH_GAP)[0].tolist())
    return bad


class Args:
    def __init__(self, k_list):
        self.inference_and_eval_setting = types.SimpleNamespace(k_list=k_list)
        self.activate_wandb = False


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
    MG._stub("wandb", log=lambda *a, **k: None, init=lambda *a, **k: None)
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
    spec = importlib.util.spec_from_file_location("ref_method_linear", os.path.join(REF, "scripts", "method_linear.py"))
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


def main():
    import contextlib
    import io

    import torch
    import torch.nn as nn

    U, R, EG = import_reference()
    args = Args(K_LIST)
    sps = species_of()
    T = torch.from_numpy
    quiet = contextlib.redirect_stdout(io.StringIO())

    # ---- the label map and the training run, both the reference's own
    train_img = synth("train_seen")[0]
    train_loader = loader_of("train_seen", train_img, BATCH, T)
    label_map, idx_to_all_labels = R.load_all_seen_species_name_and_create_label_map(train_loader)
    assert len(label_map) == CFG["n_seen_species"]
    seen0 = synth("seen_query")[0]
    val_loader0 = loader_of("seen_query", seen0, QUERY_BATCH, T)
    lin = head0()
    h0 = {"weight": lin.weight.detach().numpy().copy(), "bias": lin.bias.detach().numpy().copy()}
    model = R.ViTWIthExtraLayer(nn.Identity(), lin)
    ce = nn.CrossEntropyLoss()
    step_losses = []

    def criterion(output, target):
        loss = ce(output, target)
        step_losses.append(float(loss.item()))
        return loss

    optimizer = torch.optim.AdamW(model.parameters(), lr=LR)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=LR, total_steps=len(train_loader) * EPOCHS)
    epoch_losses, evaluation = [], []
    for _ in range(EPOCHS):
        with quiet:
            el, ev = R.fine_tuning_epoch(args, model, train_loader, val_loader0, None, optimizer, criterion, scheduler, "cpu", label_map)
        epoch_losses.append(float(el))
        evaluation.append({k: float(v) for k, v in ev.items()})
    w = model.new_linear_layer.weight.detach().numpy().copy()
    b = model.new_linear_layer.bias.detach().numpy().copy()
    print(f"trained: losses {step_losses[0]:.4f} -> {step_losses[-1]:.4f}, evaluation {evaluation[-1]}, max |w| {np.abs(w).max():.3f}")

    # ---- queries: redraw the rows that sit too close to a decision
    redraw = {"seen_query": np.zeros(CFG["n_seen"], np.int64), "unseen_query": np.zeros(CFG["n_unseen"], np.int64)}
    key_feats = {s: synth(s) for s in ("val_unseen_keys", "test_unseen_keys")}
    keys_b = np.concatenate([key_feats["val_unseen_keys"][1], key_feats["test_unseen_keys"][1]])
    for _ in range(40):
        todo = {s: bad_rows(synth(s, redraw[s])[0], w, b, keys_b) for s in redraw}
        if not any(todo.values()):
            break
        for s, rows in todo.items():
            for r in rows:
                redraw[s][r] += 1
    else:
        raise RuntimeError("probability gaps / threshold distances not reached")
    feats = {s: synth(s, redraw.get(s)) for s in SPLITS}
    loaders = {s: loader_of(s, feats[s][0], QUERY_BATCH, T) for s in SPLITS}

    def fake_get_feature_and_label(dataloader, model, device, **kw):
        img, dna = feats[dataloader.name]
        return ([f"{dataloader.name}{i}" for i in range(len(img))], img.astype(np.float64), dna.astype(np.float64), None,
                labels_of(sps[dataloader.name]))

    R.get_feature_and_label = fake_get_feature_and_label
    vocab = [{taxonomy(s)[lv]: None for s in range(CFG["n_species"])} for lv in LEVELS]
    vocab = [{x: i for i, x in enumerate(v)} for v in vocab]

    with quiet:
        final_eval = R.evaluate_epoch(model, loaders["seen_query"], "cpu", label_map)
    final_eval = {k: float(v) for k, v in final_eval.items()}

    # ---- source A and source B, then the reference end to end
    conf, idx, preds_a, gts = {}, {}, {}, {}
    for s in ("seen_query", "unseen_query"):
        c, p, g = R.inference_with_fine_tuned_image_encoder(model, loaders[s], label_map, idx_to_all_labels, "cpu")
        conf[s] = np.asarray(c, dtype=np.float64)
        assert np.array_equal(conf[s].astype(np.float32).astype(np.float64), conf[s])
        idx[s] = np.array([[label_map[x] for x in row["species"]] for row in p], dtype=np.int16)
        preds_a[s], gts[s] = p, g
    EG.ExactIP.calls = []
    pb_s, pb_u = R.inference_with_original_image_encoder_and_dna_encoder(_Model(), loaders["seen_query"], loaders["unseen_query"],
                                                                        loaders["val_unseen_keys"], loaders["test_unseen_keys"], "cpu")
    idx_b = dict(zip(("seen_query", "unseen_query"), [c.astype(np.int16) for c in EG.ExactIP.calls]))
    with quiet:
        seen_out, unseen_out = R.method_2_inference_and_eval_for_seen_and_unseen(args, model, _Model(), loaders["seen_query"], loaders["unseen_query"],
                                                                                 loaders["val_unseen_keys"], loaders["test_unseen_keys"], label_map,
                                                                                 idx_to_all_labels, "cpu")
        at_s, at_u = R.method_2_inference_and_eval_for_seen_and_unseen(args, model, _Model(), loaders["seen_query"], loaders["unseen_query"],
                                                                       loaders["val_unseen_keys"], loaders["test_unseen_keys"], label_map,
                                                                       idx_to_all_labels, "cpu", searched_threshold=GIVEN_THRESHOLD)
    splits = [{"pred_labels_from_a": preds_a["seen_query"], "pred_confidence_from_a": conf["seen_query"].tolist(), "pred_labels_from_b": pb_s,
               "gt_labels": gts["seen_query"]},
              {"pred_labels_from_a": preds_a["unseen_query"], "pred_confidence_from_a": conf["unseen_query"].tolist(), "pred_labels_from_b": pb_u,
               "gt_labels": gts["unseen_query"]}]
    grid = np.linspace(0, 1, NUM_INTERVALS + 1)
    hits = np.zeros((len(grid), 2), dtype=np.int32)
    for t, thr in enumerate(grid):
        for s, sp in enumerate(splits):
            final, gt = R.make_final_pred(args, sp["pred_labels_from_a"], sp["pred_confidence_from_a"], sp["pred_labels_from_b"], sp["gt_labels"], threshold=thr)
            acc = R.top_k_micro_accuracy(final, gt, k_list=K_LIST)[1]["species"]
            hits[t, s] = int(round(acc * len(gt)))
            assert hits[t, s] * 1.0 / len(gt) == acc
    best = float(R.search_threshold_with_harmonic_mean(args, splits))
    assert best == float(seen_out["best_threshold"]) == float(unseen_out["best_threshold"])
    Qs, Qu = CFG["n_seen"], CFG["n_unseen"]
    curve = np.array([R.harmonic_mean([hits[t, 0] * 1.0 / Qs, hits[t, 1] * 1.0 / Qu]) for t in range(len(grid))])

    # ---- the fixture must not hide a failure
    for c in conf.values():
        assert (c > 0).all() and (c <= 1).all()
        assert np.abs(c[:, :, None] - interior_grid()[None, None, :]).min() > GAP
    t = int(np.nonzero(grid == best)[0][0])
    assert 0 < t < len(grid) - 1, "the chosen threshold is the first or the last grid point"
    assert t == int(np.argmax(curve)) and hits[t, 0] / Qs >= 0.3 and hits[t, 1] / Qu >= 0.3, (hits[t], t)
    assert len(np.unique(curve)) >= 50, len(np.unique(curve))
    mixed = sum(int(((sel > 0) & (sel < M)).sum()) for sel in ((c > best).sum(axis=1) for c in conf.values()))
    assert mixed >= 20, mixed
    median_top1 = float(np.median(np.concatenate([c[:, 0] for c in conf.values()])))
    assert 0.3 <= median_top1 <= 0.9, median_top1
    logits_max = float(np.abs(np.concatenate([feats[s][0] for s in ("seen_query", "unseen_query")]).astype(np.float64) @ w.T.astype(np.float64) + b).max())

    xk = feats["seen_query"][0][:KERNEL_ROWS]
    tk = np.array([label_map[f"s{int(s)}"] for s in sps["seen_query"][:KERNEL_ROWS]], dtype=np.int64)
    out = {"cfg": CFG, "gap": GAP, "lr": LR, "epochs": EPOCHS, "batch": BATCH, "query_batch": QUERY_BATCH, "k_list": K_LIST,
           "num_intervals": NUM_INTERVALS, "head_seed": HEAD_SEED,
           "redraw": {s: r.copy() for s, r in redraw.items()}, "species": {s: v.astype(np.int16) for s, v in sps.items()},
           "vocab": [list(v) for v in vocab], "label_map": dict(label_map), "idx_to_all_labels": {int(k): dict(v) for k, v in idx_to_all_labels.items()},
           "head0": h0, "head": {"weight": w, "bias": b},
           "step_losses": np.array(step_losses, dtype=np.float64), "epoch_losses": epoch_losses, "evaluation": evaluation, "final_evaluation": final_eval,
           "conf": {s: c.astype(np.float32) for s, c in conf.items()}, "idx": idx, "idx_b": idx_b,
           "hits": hits, "best": best, "mixed": mixed, "median_top1": median_top1, "logits_absmax": logits_max,
           "out": {"seen": pack_out(seen_out, vocab), "unseen": pack_out(unseen_out, vocab)},
           "given_threshold": GIVEN_THRESHOLD, "out_at": {"seen": pack_out(at_s, vocab), "unseen": pack_out(at_u, vocab)},
           "kernel": dict(fp64_case(xk, w, b, tk), target=tk)}
    path = os.path.join(HERE, "method_linear_golden.pt")
    torch.save(out, path)
    print(f"best {best}, mixed {mixed}, median top-1 confidence {median_top1:.3f}, max |logit| {logits_max:.2f}, distinct harmonic values "
          f"{len(np.unique(curve))}, redrawn rows {int(sum((r > 0).sum() for r in redraw.values()))}, top-1 at best "
          f"{seen_out['micro_acc'][1]['species']:.3f} / {unseen_out['micro_acc'][1]['species']:.3f}, final evaluation {final_eval}")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
