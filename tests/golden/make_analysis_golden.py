"""Generate tests/golden/analysis_golden.pt: the reference's embedding analysis (scripts/result/distribution_of_similarities.py and
scripts/result/create_confusion_matrix.py) on synthetic features (authoring container only).

    python tests/golden/make_analysis_golden.py       # needs /root/reference and sklearn; writes tests/golden/analysis_golden.pt

The two reference scripts are imported with the stub pattern of make_method_linear_golden.py: hydra, h5py, seaborn, plotly, umap and
wandb are empty modules; after the import the modules' `pd`, `plt` and `tqdm` are recorders (pd.DataFrame keeps the rows, plt.hist the
series and bins, nothing is drawn or written) and create_confusion_matrix's plot_single_confusion_matrix records its arguments.  One more
name is set in that module: `list`, to a function that sorts — its `unique_classes = list(set(...))` is in hash order, which changes from
run to run, and the project states sorted class order as its divergence.  Only data is written.  The features are regenerated from
numpy's legacy RandomState by `synth` and the recorded redraw counts (tests import this module for it).

The synthetic world: D = 64, 36 species in 19 genera, 7 families and 4 orders; order o0 holds species 0..23 and >= 80 % of the keys;
species 35 has one key, alone in its genus, family and order (a singleton cluster at every level); species 10, 13 and 16, of three
genera, carry the species string "not_classified", so the hierarchy is not nested.  Centres are sums of an order, a family, a genus and a
species direction; image and DNA features are a centre plus noise, language features a per-species direction plus a little noise, all
unit rows.  300 keys, 226 seen and 226 unseen queries (18 species each, 31 down to 1 queries per species; every species has a key).

Recorded:
  sil / sil_printed   per level sklearn's silhouette_samples (fp32) of the keys' image features, and the mean the reference's
                      calculate_silhouette_score printed
  dist                per split and per query/key modality pair (all nine), the reference's nearest same-species distance, float64 (the
                      reference's function is run four times with the modalities relabelled so that every pair passes through one of
                      its five columns)
  records_head        the first three records of the plain run (column names and values)
  hist                the counts of the four series its figure bins, from the series and bins it handed to plt.hist
  idx                 per split and modality pair the top-1 key row per query that the confusion part scores (designed_predictions: a
                      designed number of each species' queries goes to one other species, so that no selection meets a tie)
  confusion           per (split, query, key, level): the classes, sklearn's confusion_matrix, and the labels and sub-matrices the
                      reference handed to its two plots
The generator asserts the conditions that keep the fixture from hiding a failure (listed at `check_conditions`).
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
LEVELS = ["order", "family", "genus", "species"]
FEATURES = ["encoded_image_feature", "encoded_dna_feature", "encoded_language_feature"]
PAIRS = [("encoded_image_feature", "encoded_image_feature"), ("encoded_dna_feature", "encoded_dna_feature"),
         ("encoded_image_feature", "encoded_dna_feature")]
BINS = [0.0, 0.3, 0.6, 0.9, 1.2, 1.5]
D = 64
SPLITS = ("key", "seen", "unseen")
QUERY_SIZES = [31, 28, 25, 22, 19, 17, 15, 13, 11, 9, 8, 7, 6, 5, 4, 3, 2, 1]     # queries per species, in species order, per split
CFG = dict(seed=0, n_species=36, n_key=300, n_seen=sum(QUERY_SIZES), n_unseen=sum(QUERY_SIZES))
NOT_CLASSIFIED = (10, 13, 16)
EDGE_GAP = 1e-3
MIN_DISTANCE = 0.5


def taxonomy(s: int) -> dict:
    if s == 35:
        return {"order": "o3", "family": "f6", "genus": "g18", "species": "s35"}
    order = "o0" if s < 24 else ("o1" if s < 30 else "o2")
    return {"order": order, "family": f"f{s // 6}", "genus": f"g{s // 2}", "species": "not_classified" if s in NOT_CLASSIFIED else f"s{s}"}


def species_of(cfg=CFG) -> dict:
    """species index per row of every split: the seen queries are of the even species, the unseen of the odd ones (every order appears
    in both), QUERY_SIZES rows each — distinct class sizes keep the confusion matrices' counts and normalised entries apart"""
    rs = np.random.RandomState(cfg["seed"])
    S = cfg["n_species"]
    w0 = np.concatenate([np.linspace(3.0, 1.0, 24), np.full(11, 0.35)])          # species 0..34; 35 gets exactly one key
    key = np.concatenate([np.arange(S), rs.choice(S - 1, cfg["n_key"] - S, p=w0 / w0.sum())])
    rs.shuffle(key)
    seen, unseen = np.repeat(np.arange(0, S, 2), QUERY_SIZES), np.repeat(np.arange(1, S, 2), QUERY_SIZES)
    rs.shuffle(seen)
    rs.shuffle(unseen)
    return {"key": key, "seen": seen, "unseen": unseen}


def synth(split: str, redraw=None, cfg=CFG):
    """(image, dna, language) fp32 [N, D] unit rows of one split; redraw[i] counts how often row i was drawn again"""
    sp = species_of(cfg)[split]
    rs = np.random.RandomState(cfg["seed"] + 1)
    S = cfg["n_species"]
    order_c, family_c, genus_c, species_c = rs.randn(4, D), rs.randn(7, D), rs.randn(19, D), rs.randn(S, D)
    text_c = rs.randn(S, D)
    tax = [taxonomy(s) for s in range(S)]
    centre = np.stack([1.0 * order_c[int(t["order"][1:])] + 0.9 * family_c[int(t["family"][1:])] + 0.9 * genus_c[int(t["genus"][1:])]
                       + 0.8 * species_c[s] for s, t in enumerate(tax)])
    text = np.stack([0.8 * centre[s] + 1.2 * text_c[s] for s in range(S)])
    out = np.empty((3, len(sp), D), dtype=np.float32)
    for i, s in enumerate(sp):
        r = np.random.RandomState([cfg["seed"], SPLITS.index(split), i, 0 if redraw is None else int(redraw[i])])
        x = np.stack([centre[s] + 1.15 * r.randn(D), centre[s] + 0.9 * r.randn(D), text[s] + 0.45 * r.randn(D)])
        out[:, i] = (x / np.sqrt(np.sum(x * x, axis=1, keepdims=True))).astype(np.float32)
    return out[0], out[1], out[2]


def labels_of(sp):
    return [taxonomy(int(s)) for s in sp]


def nearest_all_pairs(query_dict, keys_dict):
    """fp64 [9, Nq]: the nearest same-species distance of every modality pair (the generator's own check, not what is recorded)"""
    same = np.array([l["species"] for l in query_dict["label_list"]])[:, None] == np.array([l["species"] for l in keys_dict["label_list"]])[None, :]
    out = []
    for qf in FEATURES:
        for kf in FEATURES:
            q, k = query_dict[qf].astype(np.float64), keys_dict[kf].astype(np.float64)
            d = np.sqrt(((q[:, None, :] - k[None, :, :]) ** 2).sum(axis=2))
            out.append(np.where(same, d, np.inf).min(axis=1))
    return np.array(out)


def redraw_plan(cfg=CFG):
    """redraw counts per split: key rows until no two image features lie within MIN_DISTANCE (+ 0.02), then query rows until none of
    their nine distances lies within 2 EDGE_GAP of a bin edge"""
    sps = species_of(cfg)
    redraw = {s: np.zeros(len(sps[s]), dtype=np.int64) for s in SPLITS}
    for _ in range(60):
        X = synth("key", redraw["key"], cfg)[0].astype(np.float64)
        dd = np.sqrt(np.maximum(2 - 2 * X @ X.T, 0))
        dd[np.tril_indices(len(X))] = np.inf
        bad = np.unique(np.nonzero(dd < MIN_DISTANCE + 0.02)[1])
        if len(bad) == 0:
            break
        redraw["key"][bad] += 1
    else:
        raise AssertionError("key distances not reached")
    keys_dict = make_dicts(cfg, redraw)[0]
    for split in ("seen", "unseen"):
        for _ in range(60):
            qd = make_dicts(cfg, redraw)[SPLITS.index(split)]
            v = nearest_all_pairs(qd, keys_dict)
            bad = np.nonzero(np.abs(v[:, :, None] - np.array(BINS)[None, None, :]).min(axis=(0, 2)) < 2 * EDGE_GAP)[0]
            if len(bad) == 0:
                break
            redraw[split][bad] += 1
        else:
            raise AssertionError("bin-edge distances not reached")
    return redraw


def make_dicts(cfg=CFG, redraw=None):
    """keys_dict, seen_dict, unseen_dict in the reference's layout (fp32 features)"""
    sps = species_of(cfg)
    out = []
    for split in SPLITS:
        f = synth(split, None if redraw is None else redraw[split], cfg)
        d = {name: f[i] for i, name in enumerate(FEATURES)}
        d["label_list"] = labels_of(sps[split])
        d["processed_id_list"] = [f"{split}{i}" for i in range(len(sps[split]))]
        out.append(d)
    return out


def selection_ties(cm) -> str:
    """'' if neither top-10 selection of a confusion matrix meets a tie: the ten largest diagonal counts are distinct and above the
    eleventh; with more than ten classes the ten largest off-diagonal normalised entries, and every entry the reference's loop scans
    (plus the next one), are positive and distinct"""
    cm = np.asarray(cm, dtype=np.int64)
    diag = np.sort(np.diag(cm))[::-1][:11]
    if len(set(diag[:10].tolist())) != len(diag[:10]) or (len(diag) == 11 and diag[9] == diag[10]):
        return f"diagonal {diag}"
    if len(cm) > 10:
        with np.errstate(divide="ignore", invalid="ignore"):
            cmn = np.nan_to_num(cm.astype(float) / cm.sum(axis=1, keepdims=True))
        np.fill_diagonal(cmn, -np.inf)
        flat = np.sort(cmn.ravel())[::-1]
        order = np.dstack(np.unravel_index(np.argsort(-cmn.ravel(), kind="stable"), cmn.shape))[0]
        seen, used = set(), 0
        for i, j in order:
            seen.update([int(i), int(j)])
            used += 1
            if len(seen) >= 10:
                break
        scanned = flat[:max(used + 1, 10)]
        if scanned[-1] <= 0 or len(set(scanned.tolist())) != len(scanned):
            return f"off-diagonal {scanned}"
    return ""


def designed_predictions(split: str, pair: int, cfg=CFG):
    """The top-1 key row per query of one (split, modality pair), designed rather than searched: the e_c first queries of species c
    (0 <= e_c <= n_c / 4 + 1) are sent to a key of ONE other species t_c, the rest to a key of their own species; the draw is repeated
    until no level's matrix has a tie where a selection decides.  Returns (idx int64 [Q], attempt)."""
    sps = species_of(cfg)
    q_sp, k_sp = sps[split], sps["key"]
    name = [taxonomy(s) for s in range(cfg["n_species"])]
    for attempt in range(5000):
        rs = np.random.RandomState([cfg["seed"], 7, SPLITS.index(split), pair, attempt])
        idx = np.empty(len(q_sp), dtype=np.int64)
        for c in np.unique(q_sp):
            rows = np.nonzero(q_sp == c)[0]
            others = [t for t in range(cfg["n_species"]) if name[t]["species"] != name[c]["species"]]
            t = others[rs.randint(len(others))]
            e = rs.randint(0, len(rows) // 4 + 2)
            for n, r in enumerate(rows):
                idx[r] = rs.choice(np.nonzero(k_sp == (t if n < e else c))[0])
        ok = True
        for lv in LEVELS:
            classes = sorted({name[s][lv] for s in q_sp})
            m = {x: i for i, x in enumerate(classes)}
            cm = np.zeros((len(classes), len(classes)), dtype=np.int64)
            for s, j in zip(q_sp, idx):
                pj = m.get(name[k_sp[j]][lv], -1)
                if pj >= 0:
                    cm[m[name[s][lv]], pj] += 1
            if selection_ties(cm):
                ok = False
                break
        if ok:
            return idx, attempt
    raise AssertionError("no tie-free predictions found")


def pred_dict_of(keys_dict, seen_dict, unseen_dict, idx):
    """the reference's pred_dict (top-1 label lists) from index arrays idx[split][(query, key)]"""
    pd_ = {"seen_gt_label": seen_dict["label_list"], "unseen_gt_label": unseen_dict["label_list"]}
    for q, k in PAIRS:
        pd_.setdefault(q, {})[k] = {}
        for split in ("seen", "unseen"):
            pd_[q][k][f"curr_{split}_pred_list"] = [{lv: [keys_dict["label_list"][int(j)][lv]] for lv in LEVELS} for j in idx[split][(q, k)]]
    return pd_


class _Frame:
    """pd.DataFrame as a recorder: the rows, column access, and a to_csv that writes nothing"""

    last = None

    def __init__(self, rows):
        self.rows = list(rows)
        _Frame.last = self

    def __getitem__(self, col):
        return types.SimpleNamespace(tolist=lambda: [r[col] for r in self.rows])

    def to_csv(self, *a, **k):
        pass


class _Plt:
    """matplotlib.pyplot as a recorder of hist's series and bins; every other call is a no-op"""

    def __init__(self):
        self.hists = []

    def hist(self, series, bins=None, **k):
        self.hists.append(([np.asarray(s, dtype=np.float64) for s in series], list(bins), k.get("label")))

    def __getattr__(self, name):
        return lambda *a, **k: None


class _Quiet:
    def __init__(self, it, *a, **k):
        self.it = it

    def __iter__(self):
        return iter(self.it)

    def set_description(self, *a, **k):
        pass


_REFERENCE = []


def import_reference():
    if _REFERENCE:
        return _REFERENCE
    sys.path.insert(0, HERE)
    import make_golden as MG

    MG.install_stubs()
    MG._stub("umap", UMAP=MG._Anything)
    MG._stub("hydra", main=lambda *a, **k: (lambda f: f))
    MG._stub("wandb", log=lambda *a, **k: None, init=lambda *a, **k: None)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "scripts"))
    import importlib.util

    mods = []
    for name in ("distribution_of_similarities", "create_confusion_matrix"):
        spec = importlib.util.spec_from_file_location(f"ref_{name}", os.path.join(REF, "scripts", "result", f"{name}.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    _REFERENCE.extend(mods)
    return mods


def relabelled(d, perm):
    """the dict with its three feature slots permuted: slot FEATURES[i] holds the features of FEATURES[perm[i]]"""
    out = dict(d)
    for i, name in enumerate(FEATURES):
        out[name] = d[FEATURES[perm[i]]].astype(np.float64)
    return out


# the reference's five columns as (query slot, key slot); four relabellings cover all nine pairs
COLUMNS = {"distance_for_image_to_image": (0, 0), "distance_for_dna_to_dna": (1, 1), "distance_for_image_to_dna": (0, 1),
           "distance_for_dna_to_image": (1, 0), "distance_for_image_to_language": (1, 2)}
RELABELLINGS = [(0, 1, 2), (2, 1, 0), (1, 0, 2), (2, 0, 1)]


def check_conditions(dicts, sil, dist, confusion):
    keys_dict = dicts[0]
    X = keys_dict["encoded_image_feature"].astype(np.float64)
    # features are unit rows; the smallest distance between two rows is >= 0.5 (the Gram form's cancellation stays out of the fixture)
    for d in dicts:
        for f in FEATURES:
            assert np.abs(np.sqrt((d[f].astype(np.float64) ** 2).sum(axis=1)) - 1).max() < 1e-6
    dd = np.sqrt(np.maximum(2 - 2 * X @ X.T, 0))
    np.fill_diagonal(dd, np.inf)
    assert dd.min() >= MIN_DISTANCE, dd.min()
    # every level has a singleton cluster; one order holds >= 80 % of the rows; the hierarchy is not nested
    for lv in LEVELS:
        names, counts = np.unique([l[lv] for l in keys_dict["label_list"]], return_counts=True)
        assert counts.min() == 1, lv
        if lv == "order":
            assert counts.max() >= 0.8 * len(X), counts
    genera = {l["genus"] for l in keys_dict["label_list"] if l["species"] == "not_classified"}
    assert len(genera) >= 3, genera
    # every query species has a key; no distance within 1e-3 of a bin edge
    key_species = {l["species"] for l in keys_dict["label_list"]}
    for d in dicts[1:]:
        assert {l["species"] for l in d["label_list"]} <= key_species
    for split in dist:
        for pair, v in dist[split].items():
            assert np.isfinite(v).all()
            assert np.abs(v[:, None] - np.array(BINS)[None, :]).min() >= EDGE_GAP, (split, pair)
    # no ties where the two top-10 selections decide
    for key, c in confusion.items():
        assert not selection_ties(c["cm"]), (key, selection_ties(c["cm"]))
    assert max(len(c["cm"]) for c in confusion.values()) > 10
    for lv in LEVELS:
        assert sil[lv].dtype == np.float32 and np.abs(sil[lv]).max() <= 1


def generate(cfg=CFG):
    from sklearn.metrics import silhouette_samples

    RD, RC = import_reference()
    RD.pd = types.SimpleNamespace(DataFrame=_Frame)
    RD.plt = _Plt()
    RD.tqdm = _Quiet
    recorded = []
    RC.plot_single_confusion_matrix = lambda cm, classes, title, split, query, key, level: recorded.append(
        (title.split(" at ")[0], split, query, key, level, np.array(cm, dtype=np.float64), list(classes)))
    RC.list = lambda s: sorted(s)

    redraw = redraw_plan(cfg)
    dicts = make_dicts(cfg, redraw)
    keys_dict, seen_dict, unseen_dict = dicts
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(eval_on="val"), project_root_path=os.devnull)

    # ---- silhouette: the reference's print, and sklearn's samples the way the reference calls it
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        RD.calculate_silhouette_score(args, keys_dict["encoded_image_feature"], (None, keys_dict["label_list"]))
    printed = {}
    for line, lv in zip(buf.getvalue().strip().splitlines(), LEVELS):
        assert line.startswith(f"The silhouette score for {lv} level is : "), line
        printed[lv] = float(line.split(" : ")[1])
    sil = {lv: np.asarray(silhouette_samples(keys_dict["encoded_image_feature"], [l[lv] for l in keys_dict["label_list"]])) for lv in LEVELS}

    # ---- nearest same-species key: four runs of the reference's function cover the nine pairs
    dist = {"seen": {}, "unseen": {}}
    records_head, hist = None, None
    for perm in RELABELLINGS:
        RD.plt.hists.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            RD.get_similarity_for_different_combination_of_modalities(relabelled(keys_dict, perm), relabelled(seen_dict, perm),
                                                                      relabelled(unseen_dict, perm), args)
        rows = _Frame.last.rows
        assert [r["file_name"] for r in rows] == seen_dict["processed_id_list"] + unseen_dict["processed_id_list"]
        for col, (qs, ks) in COLUMNS.items():
            pair = f"{FEATURES[perm[qs]]}_{FEATURES[perm[ks]]}"
            v = np.array([r[col] for r in rows], dtype=np.float64)
            for split, part in (("seen", v[:cfg["n_seen"]]), ("unseen", v[cfg["n_seen"]:])):
                if pair in dist[split]:
                    assert np.array_equal(dist[split][pair], part), pair
                dist[split][pair] = part
        if perm == (0, 1, 2):
            records_head = [dict(r) for r in rows[:3]]
            (series, bins, names), = RD.plt.hists
            assert bins == BINS
            hist = {n: np.histogram(s, bins=bins)[0].astype(np.int64) for n, s in zip(names, series)}
            assert {r["split"] for r in rows} == {"val_seen", "val_unseen"}
    assert all(len(dist[s]) == 9 for s in dist)

    # ---- confusion: the reference's plot_confusion_matrix on the designed top-1 predictions
    idx = {split: {pair: designed_predictions(split, p, cfg)[0] for p, pair in enumerate(PAIRS)} for split in ("seen", "unseen")}
    RC.plot_confusion_matrix(pred_dict_of(keys_dict, seen_dict, unseen_dict, idx))
    from sklearn.metrics import confusion_matrix

    confusion = {}
    for title, split, q, k, lv, sub, classes in recorded:
        c = confusion.setdefault((split, q, k, lv), {})
        c["largest" if title == "Most Common Classes" else "most_confused"] = (sub, classes)
    for (split, q, k, lv), c in confusion.items():
        gt = [g[lv] for g in (seen_dict if split == "seen" else unseen_dict)["label_list"]]
        pred = [keys_dict["label_list"][int(j)][lv] for j in idx[split][(q, k)]]
        c["labels"] = sorted(set(gt))
        c["cm"] = confusion_matrix(gt, pred, labels=c["labels"]).astype(np.int16)
        assert set(c) == {"largest", "most_confused", "labels", "cm"}
    assert len(confusion) == 2 * len(PAIRS) * len(LEVELS)
    check_conditions(dicts, sil, dist, confusion)
    return {"cfg": dict(cfg), "redraw": redraw, "bins": BINS, "edge_gap": EDGE_GAP, "sil": sil, "sil_printed": printed, "dist": dist, "records_head": records_head,
            "hist": hist, "idx": {s: {k: v.astype(np.int16) for k, v in d.items()} for s, d in idx.items()}, "confusion": confusion}


def find_seed(first=0, last=200):
    """how CFG's seed was chosen: the first one whose world passes check_conditions"""
    for seed in range(first, last):
        try:
            generate(dict(CFG, seed=seed))
            return seed
        except AssertionError as e:
            print(f"seed {seed}: {str(e)[:150]}")
    raise RuntimeError("no seed found")


def main():
    import torch

    if "--find-seed" in sys.argv:
        print("seed", find_seed())
        return
    out = generate()
    path = os.path.join(HERE, "analysis_golden.pt")
    torch.save(out, path)
    print("silhouette means", out["sil_printed"])
    print("hist", {k: v.tolist() for k, v in out["hist"].items()})
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "method_linear_golden.pt"))


if __name__ == "__main__":
    main()
