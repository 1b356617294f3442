"""Generate tests/golden/insect_golden.pt: the reference's INSECT / BZSL workflow (bioscanclip/epoch/fine_tuning_epoch.py,
scripts/BZSL/extract_feature_for_insect_dataset.py) on synthetic features (authoring container only).

    python tests/golden/make_insect_golden.py       # needs /root/reference; writes tests/golden/insect_golden.pt

The reference is imported with the stub pattern of make_method_linear_golden.py (hydra and wandb no-ops, the progress bar silenced).
Only data is written: losses, the heads before and after training, accuracy dicts, argsort indices, species and key lists, the
prototype table and its CSV text, seeds and redraw counts.  Features are regenerated from numpy's legacy RandomState by
make_method_linear_golden.synth and `proto_world` below (tests import both modules for them).

Joint fine-tuning.  The synthetic world of make_method_linear_golden: D = 128, 36 seen classes, the training split's 36 x 3 rows in
batches of 36, a row's image feature in the loader's image slot and its DNA feature in the DNA slot.  The reference's own
EncoderWithExtraLayer(nn.Identity(), nn.Linear(128, 36)) twice (heads seeded IMAGE_HEAD_SEED / DNA_HEAD_SEED), trained by its own
fine_tuning_epoch_image_and_dna under torch.optim.AdamW(lr=LR) for EPOCHS epochs, the species list its own
get_unique_species_for_seen's (Python set order of the generating process: recorded).  Recorded:
  species                 the list used                    ref_state_dict_keys   the reference module's state-dict keys
  head0 / head            {"image" | "dna": {"weight", "bias"}} before / after training
  step_summands           [steps, 2] the two criterion values of every step, step_losses [steps] their fp32 sum (what loss.item() gave)
  epoch_losses            what fine_tuning_epoch_image_and_dna returned
  evaluation              {"image" | "dna": evaluate_epoch's dict} on the 200 seen queries, argsort {"image" | "dna": int16 [200, 5]} the
                          matrices its torch.argsort(...)[:, :5] produced, eval_redraw the redraw count per query row
Prototypes.  `proto_world`: PROTO_SIZES classes of 1 .. 100 rows, labels non-dense integers, rows shuffled, float32 [N, 64] features.
The reference's own lines (the block from `dict_emb = {}` to the np.savetxt of the DNA table, read from its file at run time and
executed, never copied) give class_embed [64, C] and the exact CSV text.
key_dict / overall_acc: what the reference's construct_key_dict and its overall-accuracy statement (train_cl_on_insect_dataset.py,
extracted and executed the same way) give on `key_dict_inputs()` and `overall_acc_input()`.
The generator asserts what keeps the fixture honest: for at least half of the classes with three or more rows, summing in reversed
order changes at least one bit of the mean; in every evaluated row neighbouring values of the top-6 logits lie at least LOGIT_GAP =
1e-3 apart (more than ten times the 6.3e-5 worst |logit - fp64| measured for the split product) — a row that fails is redrawn, the
redraw recorded, redraws below 5 % of the rows; the final loss is below a tenth of the first.
"""
import io
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
import make_method_linear_golden as MLG  # noqa: E402

D = MLG.D
N_CLASSES = MLG.CFG["n_seen_species"]
BATCH = 36
QUERY_BATCH = 64
LR = 0.05
EPOCHS = 40
IMAGE_HEAD_SEED, DNA_HEAD_SEED = 11, 12
K_VALUES = [1, 3, 5]
LOGIT_GAP = 1e-3
PROTO_SEED = 77
PROTO_D = 64
PROTO_SIZES = list(range(1, 33)) + [40, 48, 64, 80, 100, 1, 2, 5]


def heads0():
    """the two heads before training: nn.Linear(128, 36) under torch.manual_seed(IMAGE_HEAD_SEED / DNA_HEAD_SEED)"""
    import torch

    out = {}
    for name, seed in (("image", IMAGE_HEAD_SEED), ("dna", DNA_HEAD_SEED)):
        torch.manual_seed(seed)
        out[name] = torch.nn.Linear(D, N_CLASSES)
    return out


def joint_loader(split: str, batch: int, to_tensor, redraw=None):
    """the reference's 7-tuples of one split: image features in slot 1, DNA features in slot 2"""
    img, dna = MLG.synth(split, redraw)
    sp = MLG.species_of()[split]
    out = []
    for b0 in range(0, len(sp), batch):
        rows = slice(b0, b0 + batch)
        out.append(([f"{split}{i}" for i in range(b0, min(b0 + batch, len(sp)))], to_tensor(img[rows]), to_tensor(dna[rows]), None, None, None,
                    MLG.label_batch_of(sp[rows])))
    return MLG.Loader(split, out)


def proto_world():
    """(features float32 [N, PROTO_D], labels int64 [N]): class j has PROTO_SIZES[j] rows and the label 3 j + 5, rows shuffled"""
    rs = np.random.RandomState(PROTO_SEED)
    labels = np.concatenate([np.full(n, 3 * j + 5, dtype=np.int64) for j, n in enumerate(PROTO_SIZES)])
    rs.shuffle(labels)
    feats = (rs.randn(len(labels), PROTO_D) * np.exp(rs.randn(len(labels), 1))).astype(np.float32)
    return feats, labels


class _Quiet:                       # the reference's progress bar, silenced
    def __init__(self, it, *a, **k):
        self.it = it

    def __iter__(self):
        return iter(self.it)

    def set_description(self, *a, **k):
        pass


def reference_prototype_lines() -> str:
    """the block of extract_feature_for_insect_dataset.py that builds class_embed and writes the DNA table, dedented"""
    lines = open(os.path.join(REF, "scripts", "BZSL", "extract_feature_for_insect_dataset.py")).read().splitlines()
    first = next(i for i, l in enumerate(lines) if l.strip() == "dict_emb = {}")
    last = next(i for i, l in enumerate(lines) if i > first and "np.savetxt(dna_embed_path" in l)
    while not lines[last].rstrip().endswith(")"):
        last += 1
    return textwrap.dedent("\n".join(lines[first:last + 1]))


def reference_train_cl_lines():
    """(the source of construct_key_dict, the statement that computes overall_acc) of train_cl_on_insect_dataset.py, dedented"""
    lines = open(os.path.join(REF, "scripts", "BZSL", "train_cl_on_insect_dataset.py")).read().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith("def construct_key_dict"))
    last = next(i for i, l in enumerate(lines) if i > first and l.strip() == "return key_dict")
    o0 = next(i for i, l in enumerate(lines) if l.strip().startswith("overall_acc = ("))
    o1 = next(i for i, l in enumerate(lines) if i >= o0 and l.rstrip().endswith("/ 2"))
    return "\n".join(lines[first:last + 1]), textwrap.dedent("\n".join(lines[o0:o1 + 1]))


def key_dict_inputs():
    """four small split dictionaries in the shape get_features_and_label returns them (float32 features, every tower present)"""
    rs = np.random.RandomState(PROTO_SEED + 1)
    out = []
    for s, n in enumerate((3, 2, 4, 1)):
        labels = [MLG.taxonomy(int(x)) for x in rs.randint(0, 9, n)]
        out.append({"file_name_list": [f"f{s}_{i}" for i in range(n)], "encoded_dna_feature": rs.randn(n, 4).astype(np.float32),
                    "encoded_image_feature": rs.randn(n, 4).astype(np.float32), "encoded_language_feature": rs.randn(n, 4).astype(np.float32),
                    "averaged_feature": rs.randn(n, 4).astype(np.float32), "concatenated_feature": rs.randn(n, 8).astype(np.float32),
                    "label_list": labels, "all_key_features": rs.randn(3 * n, 4).astype(np.float32), "all_key_features_label": labels * 3})
    return out


def overall_acc_input():
    split = lambda a: {"micro_acc": {1: {"species": a, "genus": 0.9}, 3: {"species": 0.99, "genus": 1.0}}, "macro_acc": {1: {"species": 0.1, "genus": 0.2}}}
    return {"encoded_image_feature": {"encoded_image_feature": {"seen_val": split(0.625), "unseen_val": split(0.1875)},
                                      "encoded_dna_feature": {"seen_val": split(0.5), "unseen_val": split(0.25)}}}


def gap_bad_rows(feats, w, b) -> set:
    """rows whose top-6 logits (fp32, as the reference computes them) hold two neighbours closer than LOGIT_GAP"""
    import torch
    import torch.nn.functional as F

    with torch.no_grad():
        logits = F.linear(torch.from_numpy(feats), torch.from_numpy(w), torch.from_numpy(b)).numpy().astype(np.float64)
    top = np.sort(logits, axis=1)[:, ::-1][:, :6]
    return set(np.nonzero((top[:, :-1] - top[:, 1:]).min(axis=1) < LOGIT_GAP)[0].tolist())


def main():
    import contextlib
    import types

    import torch
    import torch.nn as nn

    U, _, _ = MLG.import_reference()
    import bioscanclip.epoch.fine_tuning_epoch as FT

    FT.tqdm = _Quiet
    U.tqdm = _Quiet
    args = types.SimpleNamespace(activate_wandb=False)
    T = torch.from_numpy
    quiet = contextlib.redirect_stdout(io.StringIO())

    # ---- the joint fine-tuning, the reference's own
    train_loader = joint_loader("train_seen", BATCH, T)
    species = U.get_unique_species_for_seen(train_loader)
    assert len(species) == N_CLASSES
    lins = heads0()
    h0 = {m: {"weight": l.weight.detach().numpy().copy(), "bias": l.bias.detach().numpy().copy()} for m, l in lins.items()}
    image_classifier = U.EncoderWithExtraLayer(nn.Identity(), lins["image"])
    dna_classifier = U.EncoderWithExtraLayer(nn.Identity(), lins["dna"])
    ref_keys = list(U.EncoderWithExtraLayer(nn.Linear(2, 2), nn.Linear(2, 2)).state_dict().keys())
    ce = nn.CrossEntropyLoss()
    summands = []

    def criterion(output, target):
        loss = ce(output, target)
        summands.append(float(loss.item()))
        return loss

    optimizer = torch.optim.AdamW(list(image_classifier.parameters()) + list(dna_classifier.parameters()), lr=LR)
    epoch_losses = []
    for epoch in range(EPOCHS):
        with quiet:
            epoch_losses.append(float(FT.fine_tuning_epoch_image_and_dna(args, image_classifier, dna_classifier, train_loader, optimizer, criterion,
                                                                         species, epoch, "cpu")))
    summands = np.array(summands, dtype=np.float64).reshape(-1, 2)
    step_losses = (summands[:, 0].astype(np.float32) + summands[:, 1].astype(np.float32)).astype(np.float64)
    assert len(step_losses) == EPOCHS * len(train_loader)
    assert np.allclose(step_losses.reshape(EPOCHS, -1).mean(axis=1), epoch_losses, rtol=1e-6)
    assert step_losses[-1] < 0.1 * step_losses[0], (step_losses[0], step_losses[-1])
    head = {m: {"weight": l.weight.detach().numpy().copy(), "bias": l.bias.detach().numpy().copy()} for m, l in lins.items()}

    # ---- the evaluation rows: redraw what sits too close to a swap in either modality
    n_q = MLG.CFG["n_seen"]
    redraw = np.zeros(n_q, np.int64)
    for _ in range(40):
        img, dna = MLG.synth("seen_query", redraw)
        bad = gap_bad_rows(img, head["image"]["weight"], head["image"]["bias"]) | gap_bad_rows(dna, head["dna"]["weight"], head["dna"]["bias"])
        if not bad:
            break
        for r in bad:
            redraw[r] += 1
    else:
        raise RuntimeError("logit gaps not reached")
    assert (redraw > 0).sum() < 0.05 * n_q, int((redraw > 0).sum())
    eval_loader = joint_loader("seen_query", QUERY_BATCH, T, redraw)
    evaluation, argsorts = {}, {}
    orig_argsort = torch.argsort
    for modality, clf in (("image", image_classifier), ("dna", dna_classifier)):
        rec = []

        def recording(*a, **k):
            rec.append(orig_argsort(*a, **k))
            return rec[-1]

        torch.argsort = recording
        try:
            with quiet:
                ev = FT.evaluate_epoch(clf, eval_loader, "cpu", species, modality=modality)
        finally:
            torch.argsort = orig_argsort
        evaluation[modality] = {k: float(v) for k, v in ev.items()}
        argsorts[modality] = torch.cat([r[:, :max(K_VALUES)] for r in rec]).numpy().astype(np.int16)
        assert argsorts[modality].shape == (n_q, max(K_VALUES))
    target = np.array([species.index(f"s{int(s)}") for s in MLG.species_of()["seen_query"]])
    for m in evaluation:
        assert evaluation[m]["top1_accuracy"] == float(np.mean(argsorts[m][:, 0] == target))

    # ---- the prototypes: the reference's own lines on proto_world
    feats, labels = proto_world()
    all_label = np.unique(labels)
    all_label.sort()
    buf = io.StringIO()
    ns = {"np": np, "tqdm": _Quiet, "labels": labels, "dna_feature": feats, "all_label": all_label, "dna_embed_path": buf, "print": lambda *a, **k: None}
    exec(compile(reference_prototype_lines(), "reference_prototype_lines", "exec"), ns)
    class_embed = np.asarray(ns["class_embed"], dtype=np.float32)
    assert class_embed.shape == (PROTO_D, len(PROTO_SIZES)) and np.array_equal(class_embed.astype(object), ns["class_embed"])
    assert min(PROTO_SIZES) == 1 and max(PROTO_SIZES) >= 64
    changed = total = 0
    for j, c in enumerate(all_label):
        rows = feats[labels == c]
        if len(rows) < 3:
            continue
        total += 1
        acc = rows[-1].copy()
        for r in rows[-2::-1]:
            acc = acc + r
        changed += int(not np.array_equal(acc / np.float32(len(rows)), class_embed[:, j]))
    assert changed >= total / 2, (changed, total)

    # ---- construct_key_dict and the overall accuracy: the reference's own lines again
    ckd_src, overall_src = reference_train_cl_lines()
    ns2 = {"np": np}
    exec(compile(ckd_src, "reference_construct_key_dict", "exec"), ns2)
    key_dict = ns2["construct_key_dict"](key_dict_inputs())
    ns3 = {"acc_dict": overall_acc_input()}
    exec(compile(overall_src, "reference_overall_acc", "exec"), ns3)
    assert key_dict["all_key_features"] is None and len(key_dict["label_list"]) == 10 and key_dict["encoded_dna_feature"].shape == (10, 4)

    out = {"key_dict": key_dict, "overall_acc": float(ns3["overall_acc"]), "cfg": dict(MLG.CFG), "lr": LR, "epochs": EPOCHS, "batch": BATCH, "query_batch": QUERY_BATCH, "k_values": K_VALUES, "logit_gap": LOGIT_GAP,
           "head_seeds": (IMAGE_HEAD_SEED, DNA_HEAD_SEED), "species": list(species), "ref_state_dict_keys": ref_keys,
           "head0": h0, "head": head, "step_summands": summands, "step_losses": step_losses, "epoch_losses": epoch_losses,
           "evaluation": evaluation, "argsort": argsorts, "eval_redraw": redraw.copy(),
           "proto": {"seed": PROTO_SEED, "sizes": list(PROTO_SIZES), "class_embed": class_embed, "text": buf.getvalue(),
                     "reversed_changes": (changed, total)}}
    path = os.path.join(HERE, "insect_golden.pt")
    torch.save(out, path)
    print(f"losses {step_losses[0]:.4f} -> {step_losses[-1]:.4f} over {len(step_losses)} steps, evaluation {evaluation}, redrawn rows "
          f"{int((redraw > 0).sum())} of {n_q}, reversed order changes {changed} of {total} class means, CSV {len(buf.getvalue())} characters")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
