"""The eval phase on the GPU: clibd_topk_label_hits against a numpy restatement, clibd_eval_pair_features, and the drop-in
inference_and_print_result / get_features_and_label / eval_phase / top_k_*_accuracy against the reference's recorded tables
(tests/golden/eval_golden.pt, made by tests/golden/make_eval_golden.py)."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
LEVELS = ["order", "family", "genus", "species"]
QT = ["encoded_image_feature", "encoded_dna_feature", "encoded_language_feature", "averaged_feature", "concatenated_feature"]


def _gen():
    spec = importlib.util.spec_from_file_location("make_eval_golden", ROOT / "tests" / "golden" / "make_eval_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "eval_golden.pt", weights_only=False)


# ------------------------------------------------------------------------------------------------------------------ the kernel
def restated(idx, key_ids, q_ids, off, k_list, seg, nseg):
    Q, kmax = idx.shape
    L = key_ids.shape[1]
    kl = key_ids[idx]                                                  # [Q, kmax, L]
    match = kl == q_ids[:, None, :]
    first = np.where(match.any(axis=1), match.argmax(axis=1), kmax).astype(np.int32)     # [Q, L]
    C = off[-1]
    cls = q_ids + np.asarray(off[:-1])[None, :]
    lh = np.zeros((nseg, len(k_list), L), np.int64)
    ch = np.zeros((nseg, len(k_list), C), np.int64)
    cc = np.zeros((nseg, C), np.int64)
    for s in range(nseg):
        sel = seg == s
        cc[s] = np.bincount(cls[sel].ravel(), minlength=C)
        for j, k in enumerate(k_list):
            h = first[sel] < k
            lh[s, j] = h.sum(axis=0)
            ch[s, j] = np.bincount(cls[sel].ravel(), weights=h.ravel(), minlength=C)
    return first, lh, ch, cc


def hierarchy(species):
    """species id -> [order, family, genus, species] ids (27 / 9 / 3 species per order / family / genus)"""
    s = np.asarray(species, dtype=np.int64)
    return np.stack([s // 27, s // 9, s // 3, s], axis=1).astype(np.int32)


def make_case(rs, Q, Nk, n_species, kmax, absent=True, single=False):
    key_sp = rs.randint(0, n_species, Nk)
    idx = rs.randint(0, Nk, (Q, kmax)).astype(np.int64)
    q_sp = np.where(rs.rand(Q) < 0.6, key_sp[idx[np.arange(Q), rs.randint(0, kmax, Q)]], rs.randint(0, n_species, Q))
    if absent:
        q_sp[rs.rand(Q) < 0.1] = n_species + rs.randint(0, 50)          # species (and often genera) no key has
    if single:
        key_sp[:] = 5
        q_sp[:] = 5
    key_ids, q_ids = hierarchy(key_sp), hierarchy(q_sp)
    n = np.maximum(key_ids.max(axis=0), q_ids.max(axis=0)) + 1
    off = [0] + np.cumsum(n).tolist()
    return idx, key_ids, q_ids, off


@pytest.mark.parametrize("Q", [1, 777, 50000])
@pytest.mark.parametrize("k_list", [[1], [1, 3, 5], [1, 2, 4, 8]])
@pytest.mark.parametrize("segmented", [False, True])
def test_label_hits_equal_numpy(dev, Q, k_list, segmented):
    from clibd_amd import ops

    rs = np.random.RandomState(Q * 31 + len(k_list) + 7 * segmented)
    kmax = 8 if k_list[-1] == 8 else k_list[-1] + (Q % 2)            # kmax > max(k_list) too
    idx, key_ids, q_ids, off = make_case(rs, Q, 21118, 8000, kmax)
    seg = rs.randint(0, 2, Q).astype(np.int32) if segmented else np.zeros(Q, np.int32)
    nseg = 2 if segmented else 1
    out = ops.topk_label_hits(torch.from_numpy(idx).to(dev), torch.from_numpy(key_ids).to(dev), torch.from_numpy(q_ids).to(dev), off, k_list,
                              segment=torch.from_numpy(seg).to(dev) if segmented else None, nseg=nseg)
    want = restated(idx, key_ids, q_ids, off, k_list, seg, nseg)
    for got, ref, name in zip(out, want, ("first_hit", "level_hits", "class_hits", "class_count")):
        assert np.array_equal(got.cpu().numpy(), ref), name
    if Q == 50000:
        assert want[1].sum() > 0 and (want[0] == kmax).any()          # both hits and misses exercised


def test_label_hits_single_class_and_absent_labels(dev):
    from clibd_amd import ops

    rs = np.random.RandomState(3)
    for single in (True, False):
        idx, key_ids, q_ids, off = make_case(rs, 999, 300, 40, 5, single=single)
        if not single:
            q_ids[:, 3] = off[4] - off[3] - 1            # every query's species: the last id, which no key has
            key_ids[:, 3] = np.minimum(key_ids[:, 3], off[4] - off[3] - 2)
        out = ops.topk_label_hits(torch.from_numpy(idx).to(dev), torch.from_numpy(key_ids).to(dev), torch.from_numpy(q_ids).to(dev), off, [1, 3, 5])
        want = restated(idx, key_ids, q_ids, off, [1, 3, 5], np.zeros(999, np.int32), 1)
        for got, ref in zip(out, want):
            assert np.array_equal(got.cpu().numpy(), ref)
        if single:
            assert (want[0] == 0).all()
        else:
            assert want[1][0, :, 3].sum() == 0 and (want[0][:, 3] == 5).all()


def test_label_hits_repeat_bit_identical(dev):
    from clibd_amd import ops

    rs = np.random.RandomState(9)
    idx, key_ids, q_ids, off = make_case(rs, 50000, 21118, 8000, 8)
    seg = torch.from_numpy(rs.randint(0, 2, 50000).astype(np.int32)).to(dev)
    args = [torch.from_numpy(a).to(dev) for a in (idx, key_ids, q_ids)]
    a = ops.topk_label_hits(*args, off, [1, 2, 4, 8], segment=seg, nseg=2)
    b = ops.topk_label_hits(*args, off, [1, 2, 4, 8], segment=seg, nseg=2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_label_hits_out_of_range_index_raises(dev):
    from clibd_amd import ops

    rs = np.random.RandomState(4)
    idx, key_ids, q_ids, off = make_case(rs, 100, 500, 40, 5)
    for bad in (500, -1):
        idx2 = idx.copy()
        idx2[37, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.topk_label_hits(torch.from_numpy(idx2).to(dev), torch.from_numpy(key_ids).to(dev), torch.from_numpy(q_ids).to(dev), off, [1, 3, 5])
    q2 = q_ids.copy()
    q2[5, 1] = off[2] - off[1]                       # one past the family ids
    with pytest.raises(ValueError, match="class range"):
        ops.topk_label_hits(torch.from_numpy(idx).to(dev), torch.from_numpy(key_ids).to(dev), torch.from_numpy(q2).to(dev), off, [1, 3, 5])
    seg = torch.full((100,), 2, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="segment"):
        ops.topk_label_hits(torch.from_numpy(idx).to(dev), torch.from_numpy(key_ids).to(dev), torch.from_numpy(q_ids).to(dev), off, [1, 3, 5],
                            segment=seg, nseg=2)


def test_pair_features_match_numpy(dev):
    from clibd_amd import ops

    g = torch.Generator().manual_seed(0)
    img, dna = torch.randn(1003, 768, generator=g), torch.randn(1003, 768, generator=g)
    avg, cat = ops.eval_pair_features(img.to(dev), dna.to(dev))
    ref_avg = np.mean([img.numpy().astype(np.float64), dna.numpy().astype(np.float64)], axis=0)
    assert np.abs(avg.cpu().numpy() - ref_avg).max() <= 1e-6
    assert np.array_equal(avg.cpu().numpy(), ref_avg.astype(np.float32))       # one rounding of the exact mean
    assert torch.equal(cat.cpu(), torch.cat([img, dna], dim=1))


# ------------------------------------------------------------------------------------------------------------ the drop-in API
def golden_dicts(name, golden, dev):
    """the golden set's keys / seen / unseen dictionaries as get_features_and_label(as_numpy=False) builds them"""
    from clibd_amd import ops

    gen = _gen()
    g = golden[name]
    out = {}
    for s in ("keys", "seen", "unseen"):
        img, dna, txt = (torch.from_numpy(f).to(dev) for f in gen.synth_split(g["cfg"], s, g["redraw"].get(s)))
        labels = [gen.taxonomy(int(x)) for x in g["species"][s]]
        avg, cat = ops.eval_pair_features(img, dna)
        d = {"file_name_list": [f"{s}{i}" for i in range(len(labels))], "encoded_dna_feature": dna, "encoded_image_feature": img,
             "encoded_language_feature": txt, "averaged_feature": avg, "concatenated_feature": cat, "label_list": labels,
             "all_key_features": None, "all_key_features_label": None}
        if s == "keys":
            d["all_key_features"] = torch.cat([img, dna, txt])
            d["all_key_features_label"] = labels + labels + labels
        out[s] = d
    return out


@pytest.mark.parametrize("name", ["small", "large"])
def test_inference_equals_reference(dev, golden, name):
    from clibd_amd import eval as E

    g = golden[name]
    d = golden_dicts(name, golden, dev)
    if name == "large":
        assert d["keys"]["encoded_image_feature"].shape[0] >= 4096       # every key type takes the pre-filtered search
    acc, per_class, pred = E.inference_and_print_result(d["keys"], d["seen"], d["unseen"], k_list=g["k_list"])
    assert acc == g["acc_dict"]
    assert per_class == g["per_class_acc"]
    assert E.compute_overall_acc(acc) == g["overall_acc"]
    assert pred["seen_id"] == d["seen"]["file_name_list"] and pred["unseen_gt_label"] == d["unseen"]["label_list"]
    vocab = [{x: i for i, x in enumerate(v)} for v in g["vocab"]]
    n = 0
    for qt in QT:
        for kt, pr in pred[qt].items():
            if not pr:
                assert (qt, kt) not in g["pred_codes"]
                continue
            for lst, want in zip((pr["curr_seen_pred_list"], pr["curr_unseen_pred_list"]), g["pred_codes"][(qt, kt)]):
                got = np.array([[[vocab[l][x] for x in p[lv]] for l, lv in enumerate(LEVELS)] for p in lst])
                assert np.array_equal(got, want), (qt, kt)
            n += 1
    assert n == len(g["pred_codes"])
    _, _, pred_i = E.inference_and_print_result(d["keys"], d["seen"], d["unseen"], k_list=g["k_list"], with_predictions=False)
    for (qt, kt), (s_idx, u_idx) in g["pred_idx"].items():
        assert pred_i[qt][kt]["curr_seen_pred_list"].dtype == np.int64
        assert np.array_equal(pred_i[qt][kt]["curr_seen_pred_list"], s_idx) and np.array_equal(pred_i[qt][kt]["curr_unseen_pred_list"], u_idx), (qt, kt)


def test_pair_features_match_reference_construction(dev, golden):
    g = golden["small"]
    d = golden_dicts("small", golden, dev)["keys"]
    head = g["construct_head"]
    assert np.abs(d["averaged_feature"][:5].cpu().numpy() - head["averaged_feature"]).max() <= 1e-6
    assert np.array_equal(d["concatenated_feature"][:5].cpu().numpy(), head["concatenated_feature"])
    assert head["all_key_features_label"] == d["all_key_features_label"][:5]


def test_top_k_accuracy_equals_reference(dev, golden):
    from clibd_amd import eval as E

    g = golden["standalone"]
    gt = [{lv: f"{lv[0]}{g['gt'][q, l]}" for l, lv in enumerate(LEVELS)} for q in range(len(g["gt"]))]
    pr = [{lv: [f"{lv[0]}{x}" for x in g["preds"][q, l]] for l, lv in enumerate(LEVELS)} for q in range(len(g["gt"]))]
    assert E.top_k_micro_accuracy(pr, gt, g["k_list"]) == g["micro"]
    macro, per_class = E.top_k_macro_accuracy(pr, gt, g["k_list"])
    assert macro == g["macro"] and per_class == g["per_class"]
    # k beyond the lists' length: the whole list (pred[level][:k])
    short = [{lv: p[lv][:3] for lv in LEVELS} for p in pr]
    m5 = E.top_k_micro_accuracy(short, gt, [1, 5])
    assert m5[5] == E.top_k_micro_accuracy(short, gt, [3])[3]


# --------------------------------------------------------------------------------------------------------- a tiny model end to end
def tiny_model(dev):
    from clibd_amd.model import (BertConfigLite, BertForMaskedLM, BertModel, CLIBDDNAEncoder, CLIBDImageEncoder, CLIBDLanguageEncoder, SimpleCLIP,
                                 VisionTransformer)

    tiny = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)
    torch.manual_seed(0)
    model = SimpleCLIP(
        CLIBDImageEncoder(VisionTransformer(embed_dim=128, depth=2, num_heads=2, num_classes=10), 4, 128),
        CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=1027, **tiny)), 4, 128),
        CLIBDLanguageEncoder(BertModel(BertConfigLite(vocab_size=1000, **tiny)), 4, 128),
    )
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0, 0.05)
    return model.to(dev)


def loader(seed, n_batches, B=8):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(n_batches):
        sp = torch.randint(0, 12, (B,), generator=g).tolist()
        labels = {"order": [f"o{s // 9}" for s in sp], "family": [f"f{s // 3}" for s in sp], "genus": [f"g{s // 2}" for s in sp],
                  "species": [f"s{s}" for s in sp]}
        ids = torch.randint(0, 1000, (B, 20), generator=g)
        out.append(([f"p{seed}_{b}_{i}" for i in range(B)], torch.rand(B, 3, 224, 224, generator=g),
                    torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, 1027, (B, 132), generator=g)], dim=1),
                    ids, torch.zeros_like(ids), torch.ones_like(ids), labels))
    return out


def test_get_features_and_label_tiny_model(dev):
    from clibd_amd import eval as E

    model = tiny_model(dev)
    dl = loader(1, 2)
    d = E.get_features_and_label(dl, model, dev, for_key_set=True)
    img, dna, txt = d["encoded_image_feature"], d["encoded_dna_feature"], d["encoded_language_feature"]
    assert img.dtype == np.float32 and img.shape == (16, 128)
    ref_avg = np.mean([img.astype(np.float64), dna.astype(np.float64)], axis=0)
    assert np.abs(d["averaged_feature"] - ref_avg).max() <= 1e-6
    assert np.abs(d["concatenated_feature"] - np.concatenate((img, dna), axis=1)).max() <= 1e-6
    assert np.array_equal(d["all_key_features"], np.concatenate((img, dna, txt), axis=0))
    assert d["all_key_features_label"] == d["label_list"] * 3 and len(d["label_list"]) == 16
    assert d["file_name_list"][0] == "p1_0_0"
    q = E.get_features_and_label(dl, model, dev)
    assert q["all_key_features"] is None and q["all_key_features_label"] is None
    t = E.get_features_and_label(dl, model, dev, for_key_set=True, as_numpy=False)
    assert t["averaged_feature"].is_cuda and torch.equal(t["averaged_feature"].cpu(), torch.from_numpy(d["averaged_feature"]))


def test_eval_phase_tiny_model(dev):
    from clibd_amd import eval as E

    model = tiny_model(dev)
    keys_dl, seen_dl, unseen_dl = loader(2, 3), loader(3, 2), loader(4, 2)
    acc, pred = E.eval_phase(model, dev, keys_dl, seen_dl, unseen_dl, [1, 3, 5])
    # the same functions fed host data (numpy features, the reference's convention)
    host = [E.get_features_and_label(dl, model, dev, for_key_set=(i == 0)) for i, dl in enumerate((keys_dl, seen_dl, unseen_dl))]
    acc_h, _, pred_h = E.inference_and_print_result(*host, k_list=[1, 3, 5])
    assert acc == acc_h and pred == pred_h
    assert set(acc) == set(QT) and set(acc["encoded_image_feature"]) == set(QT + ["all_key_features"])
    assert acc["concatenated_feature"]["encoded_image_feature"] == {}          # width mismatch: skipped, as in the reference
    overall = E.compute_overall_acc(acc)
    assert 0.0 <= overall <= 1.0 and overall == E.compute_overall_acc(acc_h)
    with pytest.raises(NotImplementedError):
        E.eval_phase(model, dev, keys_dl, seen_dl, unseen_dl, [1], for_open_clip=True)
