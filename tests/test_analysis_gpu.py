"""GPU checks of the embedding analysis (clibd_amd.analysis, include/clibd_hip_analysis.h): the silhouette kernel against the fp64
restatement of tests/analysis_reference.py, gated per sample at 4 x the error of the fp32 same-formula emulation on the same inputs (the
margin covers the different summation order); the nearest same-label key against the fp64 difference form at the fp32 accumulation
bound D 2^-24; the confusion counts and every reference-named function against tests/golden/analysis_golden.pt.

Measured on an MI355X (max |s_device - s_fp64| / gate): see DESIGN §3.9."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import analysis_reference as AR  # noqa: E402

pytestmark = pytest.mark.gpu
LEVELS = ["order", "family", "genus", "species"]


def gen_module():
    spec = importlib.util.spec_from_file_location("make_analysis_golden", ROOT / "tests" / "golden" / "make_analysis_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "analysis_golden.pt", weights_only=False)


@pytest.fixture(scope="module")
def world(golden):
    G = gen_module()
    return G, G.make_dicts(golden["cfg"], golden["redraw"])


def clustered(N, D, C, seed, dominant=False):
    """unit rows around C centres; codes cover every cluster; with `dominant` cluster 0 holds about 80 % of the rows"""
    rs = np.random.RandomState(seed)
    if C == N - 1:
        codes = np.arange(N)
        codes[-1] = 0
    elif dominant:
        codes = np.where(rs.rand(N) < 0.8, 0, rs.randint(1, C, N))
    else:
        codes = rs.randint(0, C, N)
    codes[:C] = np.arange(C) if C < N - 1 else codes[:C]
    rs.shuffle(codes)
    x = rs.randn(C, D)[codes] + 0.9 * rs.randn(N, D)
    x = (x / np.sqrt((x * x).sum(axis=1, keepdims=True))).astype(np.float32)
    return x, codes.astype(np.int64)


_refs = {}


def reference(key, x, codes):
    """(fp64 silhouette, gate) of one input, computed once: gate = 4 x the fp32 emulation's max error against fp64"""
    if key not in _refs:
        s64 = AR.silhouette_fp64(x, codes)
        emu = np.abs(AR.silhouette_fp32_gram(x, codes).astype(np.float64) - s64).max()
        _refs[key] = (s64, 4.0 * emu)
    return _refs[key]


CASES = {
    "130x64_c4": dict(N=130, D=64, C=4),
    "257x128_c7": dict(N=257, D=128, C=7),
    "513x128_c127": dict(N=513, D=128, C=127),
    "300x768_c40": dict(N=300, D=768, C=40),
    "257_chunk64_dominant": dict(N=257, D=64, C=6, dominant=True, col_chunk=64),
    "c2": dict(N=150, D=64, C=2),
    "c_n_minus_1": dict(N=140, D=64, C=139, col_chunk=64),
    "d100_padded": dict(N=200, D=100, C=9),
}


@pytest.mark.parametrize("name", list(CASES))
def test_silhouette_against_fp64(name):
    """rows arrive unsorted: the Python form sorts, pads D and restores the caller's order"""
    from clibd_amd import analysis as A

    case = dict(CASES[name])
    chunk = case.pop("col_chunk", 0)
    x, codes = clustered(seed=len(name), **case)
    s64, gate = reference(name, x, codes)
    if case.get("dominant"):
        assert np.bincount(codes).max() >= 0.7 * len(codes) and len(A.chunk_plan(len(x), chunk)) >= 5
    s = A.silhouette_samples(torch.from_numpy(x).cuda(), codes, chunk)
    assert s.dtype == torch.float32 and s.is_cuda and s.shape == (len(x),)
    s = s.cpu().numpy().astype(np.float64)
    err = np.abs(s - s64).max()
    print(f"silhouette {name}: device error {err:.3e}, gate {gate:.3e}")
    assert np.isfinite(s).all() and err <= gate
    counts = np.bincount(codes)
    assert (s[counts[codes] == 1] == 0).all()


def test_silhouette_sorted_rows_through_ops_and_bit_identical():
    from clibd_amd import analysis as A
    from clibd_amd import ops

    x, codes = clustered(257, 128, 7, seed=5, dominant=True)
    order, seg = A.plan_clusters(codes)
    xs = torch.from_numpy(x[order]).cuda()
    s64, gate = reference("ops257", x[order], codes[order])
    outs = [ops.silhouette_samples(xs, seg, cc).cpu().numpy() for cc in (0, 64, 64, 128, 0)]
    assert np.array_equal(outs[1], outs[2]) and np.array_equal(outs[0], outs[4])          # two calls: the same bits
    for o in outs:
        assert np.abs(o.astype(np.float64) - s64).max() <= gate
    with pytest.raises(ValueError):
        ops.silhouette_samples(xs, np.array([0, 257], dtype=np.int32))
    with pytest.raises(ValueError):
        ops.silhouette_samples(xs[:, :100].contiguous(), seg)
    with pytest.raises(Exception, match="seg must rise"):
        ops.silhouette_samples(xs, np.array([0, 200, 100, 257], dtype=np.int32))


def test_silhouette_near_duplicates():
    """two identical rows and one pair 1e-4 apart in one cluster: the Gram form loses the small distances (a CPU emulation showed 1.6e-4
    per distance) but the silhouette stays within the gate, finite and in [-1, 1]"""
    from clibd_amd import analysis as A

    x, codes = clustered(200, 64, 5, seed=11)
    rows = np.nonzero(codes == 2)[0]
    x[rows[1]] = x[rows[0]]
    x[rows[3]] = x[rows[2]] + np.float32(1e-4 / 8.0)
    s64, gate = reference("dups", x, codes)
    s = A.silhouette_samples(torch.from_numpy(x).cuda(), codes).cpu().numpy().astype(np.float64)
    err = np.abs(s - s64).max()
    print(f"silhouette near-duplicates: device error {err:.3e}, gate {gate:.3e}")
    assert np.isfinite(s).all() and s.min() >= -1 and s.max() <= 1
    assert err <= gate


def nearest_case(seed, Nq=300, Nk=400, D=96, C=30):
    rs = np.random.RandomState(seed)
    centres = rs.randn(C, D)
    kc = np.sort(rs.randint(0, C, Nk))
    kc[kc == 7] = 8                                    # class 7 has no key
    qc = rs.randint(0, C, Nq).astype(np.int32)
    qc[:5] = -1
    qc[5:10] = 7
    K = (centres[kc] + rs.randn(Nk, D)).astype(np.float32)
    Q = (centres[np.maximum(qc, 0)] + rs.randn(Nq, D)).astype(np.float32)
    return Q, K, qc, kc


def test_same_label_nearest_against_fp64():
    from clibd_amd import analysis as A
    from clibd_amd import ops

    Q, K, qc, kc = nearest_case(2)
    D = Q.shape[1]
    _, seg = A.plan_groups(kc, 30)
    # a tie: the first two keys of class 3 are the same row
    first = int(seg[3])
    K[first + 1] = K[first]
    Q[20] = K[first] + np.float32(0.01)
    qc[20] = 3
    d64, arg64, second = AR.nearest_fp64(Q, K, qc, kc)
    dist, arg = ops.same_label_nearest(torch.from_numpy(Q).cuda(), torch.from_numpy(K).cuda(), seg, torch.from_numpy(qc).cuda())
    dist, arg = dist.cpu().numpy(), arg.cpu().numpy()
    none = (qc < 0) | (qc == 7)
    assert none.sum() >= 10 and np.isinf(dist[none]).all() and (dist[none] > 0).all() and (arg[none] == -1).all()
    assert np.isinf(d64[none]).all()
    bound = D * 2.0 ** -24
    rel = np.abs(dist[~none].astype(np.float64) - d64[~none]) / d64[~none]
    print(f"same_label_nearest: max relative error {rel.max():.3e}, bound {bound:.3e}")
    assert rel.max() <= bound
    sure = ~none & (second > d64 * (1 + 2 * bound))
    assert sure.sum() >= 0.99 * (~none).sum()
    assert np.array_equal(arg[sure], arg64[sure])
    assert arg[20] == first and arg64[20] == first                       # the lower row of the tie
    assert (kc[arg[~none]] == qc[~none]).all()
    # strided rows (a column slice) and the Python form with labels, keys not grouped
    perm = np.random.RandomState(0).permutation(len(K))
    wide = torch.zeros(len(Q), D + 32, device="cuda")
    wide[:, :D] = torch.from_numpy(Q)
    labels_k, labels_q = [f"c{c}" for c in kc[perm]], [f"c{c}" if c >= 0 else "none" for c in qc]
    d2, a2 = A.nearest_same_species(wide[:, :D], K[perm], labels_q, labels_k)
    assert a2.dtype == torch.int64 and np.array_equal(d2.cpu().numpy(), dist)
    a2 = a2.cpu().numpy()
    assert (a2[none] == -1).all() and np.array_equal(perm[a2[sure]], arg64[sure])
    assert perm[a2[20]] in (first, first + 1) and a2[20] == min(np.nonzero(perm == first)[0][0], np.nonzero(perm == first + 1)[0][0])


def test_confusion_counts_against_numpy(golden, world):
    from clibd_amd import ops

    rs = np.random.RandomState(4)
    for N, C in ((1, 1), (1000, 7), (5000, 130)):
        t, p = rs.randint(-1, C, N).astype(np.int32), rs.randint(-1, C, N).astype(np.int32)
        got = ops.confusion_counts(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda(), C)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), AR.confusion_np(t, p, C))
        assert int(got.sum()) == int(((t >= 0) & (p >= 0)).sum())
    G, (keys_dict, seen_dict, unseen_dict) = world
    skipped = 0
    for (split, q, k, lv), c in golden["confusion"].items():
        qd = seen_dict if split == "seen" else unseen_dict
        m = {x: i for i, x in enumerate(c["labels"])}
        t = np.array([m[g[lv]] for g in qd["label_list"]], dtype=np.int32)
        p = np.array([m.get(keys_dict["label_list"][int(j)][lv], -1) for j in golden["idx"][split][(q, k)]], dtype=np.int32)
        skipped += int((p < 0).sum())
        got = ops.confusion_counts(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda(), len(m)).cpu().numpy()
        assert np.array_equal(got, c["cm"])
    assert skipped > 0          # predictions outside the ground truth's classes occur in the fixture


def test_reference_named_functions_against_the_golden(golden, world, capsys, tmp_path):
    import types

    from clibd_amd import analysis as A

    G, (keys_dict, seen_dict, unseen_dict) = world
    # silhouette: the four printed lines, the means, the samples
    means = A.calculate_silhouette_score(None, keys_dict["encoded_image_feature"], (None, keys_dict["label_list"]))
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 4
    per_level = A.silhouette_by_level(keys_dict["encoded_image_feature"], keys_dict["label_list"], col_chunk=64)
    codes = G_codes(keys_dict["label_list"])
    for l, lv in enumerate(LEVELS):
        assert lines[l] == f"The silhouette score for {lv} level is : {means[lv]}"
        s64, gate = reference(("golden", lv), keys_dict["encoded_image_feature"], codes[:, l])
        s = per_level[lv].cpu().numpy().astype(np.float64)
        err = np.abs(s - s64).max()
        print(f"silhouette golden {lv}: device error {err:.3e}, gate {gate:.3e}, vs sklearn {np.abs(s - golden['sil'][lv]).max():.3e}")
        assert err <= gate
        assert np.abs(s - golden["sil"][lv].astype(np.float64)).max() <= gate + 5e-7
        assert abs(means[lv] - golden["sil_printed"][lv]) <= gate + 2e-6
    # nearest same-species key: records, the nine pairs, histogram counts
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(eval_on="val"), project_root_path=str(tmp_path))
    records = A.get_similarity_for_different_combination_of_modalities(keys_dict, seen_dict, unseen_dict, args)
    capsys.readouterr()
    csv_path = tmp_path / "distribution_of_similarities" / "val_query_info_with_distance_to_nearest_key_with_same_species.csv"
    assert csv_path.exists() and len(csv_path.read_text().splitlines()) == len(records) + 1
    assert len(records) == 452 and [r["file_name"] for r in records] == seen_dict["processed_id_list"] + unseen_dict["processed_id_list"]
    ref_cols = list(golden["records_head"][0])
    assert list(records[0])[:len(ref_cols)] == ref_cols and list(records[0])[len(ref_cols):] == [A.TRUE_IMAGE_TO_LANGUAGE]
    for r, g in zip(records, golden["records_head"]):
        for k, v in g.items():
            assert r[k] == v if isinstance(v, str) else abs(r[k] - v) <= 64 * 2.0 ** -24 * v
    img, dna, lang = G.FEATURES
    cols = {"distance_for_image_to_image": (img, img), "distance_for_dna_to_dna": (dna, dna), "distance_for_image_to_dna": (img, dna),
            "distance_for_dna_to_image": (dna, img), "distance_for_image_to_language": (dna, lang), A.TRUE_IMAGE_TO_LANGUAGE: (img, lang)}
    bound = 64 * 2.0 ** -24
    for col, (qf, kf) in cols.items():
        ref = np.concatenate([golden["dist"]["seen"][f"{qf}_{kf}"], golden["dist"]["unseen"][f"{qf}_{kf}"]])
        got = np.array([r[col] for r in records])
        assert (np.abs(got - ref) <= bound * ref).all(), col
    assert {r["split"] for r in records} == {"val_seen", "val_unseen"}
    hist = A.distance_histograms(records)
    for name, counts in golden["hist"].items():
        assert np.array_equal(hist[name], counts), name
    klab = [l["species"] for l in keys_dict["label_list"]]
    for split, qd in (("seen", seen_dict), ("unseen", unseen_dict)):
        qlab = [l["species"] for l in qd["label_list"]]
        for qf in G.FEATURES:
            for kf in G.FEATURES:
                d, arg = A.nearest_same_species(qd[qf], keys_dict[kf], qlab, klab)
                ref = golden["dist"][split][f"{qf}_{kf}"]
                assert (np.abs(d.cpu().numpy() - ref) <= bound * ref).all(), (split, qf, kf)
                assert (np.array(klab)[arg.cpu().numpy()] == np.array(qlab)).all()
    # confusion: both prediction conventions, matrices and selections under ==
    idx_form = G.pred_dict_of(keys_dict, seen_dict, unseen_dict, golden["idx"])
    for split in ("seen", "unseen"):
        for q, k in G.PAIRS:
            idx_form[q][k][f"curr_{split}_pred_list"] = np.repeat(golden["idx"][split][(q, k)].astype(np.int64)[:, None], 5, axis=1)
    list_form = G.pred_dict_of(keys_dict, seen_dict, unseen_dict, golden["idx"])
    for result in (A.confusion_from_predictions(list_form), A.confusion_from_predictions(idx_form, keys_dict["label_list"])):
        for (split, q, k, lv), c in golden["confusion"].items():
            r = result[split][(q, k)][lv]
            assert r["labels"] == c["labels"] and r["cm"].dtype == np.int64 and np.array_equal(r["cm"], c["cm"])
            for name in ("largest", "most_confused"):
                assert r[name][1] == c[name][1] and np.array_equal(r[name][0], c[name][0]), (split, q, k, lv, name)
    (split, q, k, lv), c = next((key, c) for key, c in golden["confusion"].items() if len(c["labels"]) > 10)
    qd = seen_dict if split == "seen" else unseen_dict
    y_true = [g[lv] for g in qd["label_list"]]
    y_pred = [keys_dict["label_list"][int(j)][lv] for j in golden["idx"][split][(q, k)]]
    assert np.array_equal(A.confusion_matrix(y_true, y_pred, c["labels"]), c["cm"])
    for fn, name in ((A.largest_10_classes, "largest"), (A.most_confused_10_classes, "most_confused")):
        sub, labels = fn(y_pred, y_true, c["labels"])
        assert labels == c[name][1] and np.array_equal(sub, c[name][0])


def G_codes(label_list):
    from clibd_amd.eval import LabelCodec

    return LabelCodec().encode(label_list)
