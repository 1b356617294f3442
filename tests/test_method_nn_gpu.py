"""Seen/unseen classification by similarity threshold on the GPU: clibd_threshold_sweep_hits and clibd_threshold_merge against numpy
restatements and each other, and clibd_amd.method_nn (list and device convention) against the reference's recorded results
(tests/golden/method_nn_golden.pt, made by tests/golden/make_method_nn_golden.py)."""
import importlib.util
import types
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
LEVELS = ["order", "family", "genus", "species"]


def _gen():
    spec = importlib.util.spec_from_file_location("make_method_nn_golden", ROOT / "tests" / "golden" / "make_method_nn_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "method_nn_golden.pt", weights_only=False)


# ------------------------------------------------------------------------------------------------------------------ the kernels
def hierarchy(species):
    s = np.asarray(species, dtype=np.int64)
    return np.stack([s // 27, s // 9, s // 3, s], axis=1).astype(np.int32)


def grid_of(T):
    """T = 257: i / 256, every threshold an fp32 value (confidences EQUAL to a threshold exist); 1000 / 1001: np.linspace(0, 1, T), most
    thresholds not representable in fp32 (their fp32 neighbours lie on both sides); T = 1: [0.5]"""
    return np.array([0.5]) if T == 1 else np.linspace(0, 1, T)


def make_case(rs, Q, m, T, L=4, Nka=2111, Nkb=1500, n_species=800):
    """Two random searches like test_eval_accuracy_gpu.make_case (queries matching a returned key 60 % of the time, 10 % with a species no
    key has) and UNSORTED confidences with the edge values planted."""
    sp_a, sp_b = rs.randint(0, n_species, Nka), rs.randint(0, n_species, Nkb)
    idx_a = rs.randint(0, Nka, (Q, m)).astype(np.int64)
    idx_b = rs.randint(0, Nkb, (Q, m)).astype(np.int64)
    r = np.arange(Q)
    pick = rs.randint(0, m, Q)
    q_sp = np.where(rs.rand(Q) < 0.3, sp_a[idx_a[r, pick]], np.where(rs.rand(Q) < 0.45, sp_b[idx_b[r, pick]], rs.randint(0, n_species, Q)))
    q_sp[rs.rand(Q) < 0.1] = n_species + rs.randint(0, 50)
    la, lb, ql = (hierarchy(x)[:, 4 - L:].copy() for x in (sp_a, sp_b, q_sp))
    thr = grid_of(T)
    conf = rs.rand(Q, m).astype(np.float32)
    flat = conf.reshape(-1)
    n = flat.size
    t32 = thr[rs.randint(0, T, n)].astype(np.float32)           # the fp32 value nearest a threshold: equal to it, or a neighbour on either side
    kind = rs.randint(0, 12, n)
    flat[kind == 0] = t32[kind == 0]
    flat[kind == 1] = np.nextafter(t32, np.float32(np.inf))[kind == 1]
    flat[kind == 2] = np.nextafter(t32, np.float32(-np.inf))[kind == 2]
    special = np.array([np.nan, np.inf, -np.inf, -0.25, 1.5, -0.0, 1.0, 0.0], dtype=np.float32)
    flat[kind == 3] = special[rs.randint(0, len(special), n)][kind == 3]
    return conf, idx_a, idx_b, la, lb, ql, thr


def restated_sweep_direct(conf, idx_a, idx_b, la, lb, ql, seg, nseg, thr, k_list):
    """level_hits [T, nseg, n_k, L] in numpy, the definition as written: per position `float64(conf) > t` picks A's key label or B's,
    a hit is the query's label among the first k merged labels"""
    Q, m = conf.shape
    L = ql.shape[1]
    mA = la[idx_a] == ql[:, None, :]                             # [Q, m, L]
    mB = lb[idx_b] == ql[:, None, :]
    c = conf.astype(np.float64)
    out = np.zeros((len(thr), nseg, len(k_list), L), np.int64)
    onehot = (seg[:, None] == np.arange(nseg)[None, :]).astype(np.int64)      # [Q, nseg]
    step = max(1, 4_000_000 // (Q * m * L))
    for t0 in range(0, len(thr), step):
        with np.errstate(invalid="ignore"):
            sel = c[None, :, :] > thr[t0:t0 + step, None, None]  # [t, Q, m]
        match = np.where(sel[..., None], mA[None], mB[None])    # [t, Q, m, L]
        for i, k in enumerate(k_list):
            hit = match[:, :, :k, :].any(axis=2).astype(np.int64)            # [t, Q, L]
            out[t0:t0 + step, :, i, :] = np.einsum("tql,qs->tsl", hit, onehot)
    return out


def restated_sweep(conf, idx_a, idx_b, la, lb, ql, seg, nseg, thr, k_list):
    """the same counts with the per-position matches packed into bytes (an order of magnitude faster at 20 000 queries; the tests below
    hold it against `restated_sweep_direct` at the small sizes)"""
    Q, m = conf.shape
    L = ql.shape[1]
    bit = (1 << np.arange(m)).astype(np.uint8)
    hA = ((la[idx_a] == ql[:, None, :]) * bit[None, :, None]).sum(axis=1).astype(np.uint8)      # [Q, L]
    hB = ((lb[idx_b] == ql[:, None, :]) * bit[None, :, None]).sum(axis=1).astype(np.uint8)
    c = conf.astype(np.float64)
    onehot = (seg[:, None] == np.arange(nseg)[None, :]).astype(np.float64)    # [Q, nseg]; sums below 2^53 are exact
    out = np.zeros((len(thr), nseg, len(k_list), L), np.int64)
    step = max(1, 2_000_000 // Q)
    for t0 in range(0, len(thr), step):
        t = thr[t0:t0 + step]
        s = np.zeros((len(t), Q), np.uint8)
        with np.errstate(invalid="ignore"):
            for j in range(m):
                s |= (c[None, :, j] > t[:, None]).astype(np.uint8) << np.uint8(j)
        for l in range(L):
            merged = (s & hA[None, :, l]) | (~s & hB[None, :, l])
            for i, k in enumerate(k_list):
                hit = (merged & np.uint8((1 << k) - 1)) != 0
                out[t0:t0 + step, :, i, l] = np.rint(hit.astype(np.float64) @ onehot).astype(np.int64)
    return out


def segments(rs, Q, nseg, interleaved):
    if nseg == 1:
        return np.zeros(Q, np.int32)
    if interleaved:
        return rs.randint(0, nseg, Q).astype(np.int32)
    return np.sort(rs.randint(0, nseg, Q)).astype(np.int32)      # grouped: seen first, then unseen


def run_sweep(dev, case, seg, nseg, k_list):
    from clibd_amd import ops

    conf, idx_a, idx_b, la, lb, ql, thr = case
    d = [torch.from_numpy(a).to(dev) for a in (conf, idx_a, idx_b, la, lb, ql, thr)]
    return ops.threshold_sweep_hits(*d, k_list, segment=torch.from_numpy(seg).to(dev) if nseg > 1 else None, nseg=nseg)


SWEEP_CASES = [
    # Q, m, T, k_list, nseg, interleaved, L
    (1, 1, 1, [1], 1, False, 4),
    (1, 8, 1001, [1, 2, 4, 8], 1, False, 4),
    (777, 5, 1000, [1, 3, 5], 2, True, 4),
    (777, 8, 257, [1, 2, 4, 8], 2, False, 4),
    (777, 8, 257, [1, 3, 5], 2, True, 4),                         # m beyond max(k_list)
    (777, 1, 1001, [1], 1, False, 4),
    (777, 5, 1, [1, 3, 5], 2, True, 4),
    (777, 5, 257, [1, 3, 5], 1, False, 1),                        # one level
    (20000, 5, 1000, [1, 3, 5], 2, False, 4),
    (20000, 8, 257, [1, 2, 4, 8], 2, True, 4),
    (20000, 5, 1001, [1], 1, False, 4),
]


@pytest.mark.parametrize("Q,m,T,k_list,nseg,interleaved,L", SWEEP_CASES)
def test_sweep_equals_numpy(dev, Q, m, T, k_list, nseg, interleaved, L):
    rs = np.random.RandomState(Q * 13 + m * 7 + T + len(k_list) + nseg)
    case = make_case(rs, Q, m, T, L=L)
    seg = segments(rs, Q, nseg, interleaved)
    got = run_sweep(dev, case, seg, nseg, k_list).cpu().numpy()
    want = restated_sweep(*case[:6], seg, nseg, case[6], k_list)
    assert got.shape == want.shape and got.dtype == np.int32
    assert np.array_equal(got, want)
    if Q <= 777:
        assert np.array_equal(want, restated_sweep_direct(*case[:6], seg, nseg, case[6], k_list))
    if Q >= 777 and T >= 257:
        assert want.sum() > 0 and len(np.unique(want.reshape(T, -1).sum(axis=1))) > 10     # the counts move with the threshold
        conf, thr = case[0].astype(np.float64), case[6]
        finite = conf[np.isfinite(conf)]
        # the planted edge values exist: confidences within one fp32 ulp of a threshold, and (T = 257) equal to one
        assert (np.abs(finite[:, None] - thr[None, ::max(1, T // 16)]) < 1e-7).any()
        if T == 257:
            assert np.isin(finite, thr).sum() > 10
        assert np.isnan(case[0]).any() and np.isinf(case[0]).any()


def test_sweep_repeat_bit_identical(dev):
    rs = np.random.RandomState(21)
    case = make_case(rs, 20000, 5, 1000)
    seg = segments(rs, 20000, 2, True)
    a = run_sweep(dev, case, seg, 2, [1, 3, 5])
    b = run_sweep(dev, case, seg, 2, [1, 3, 5])
    assert torch.equal(a, b)


def test_merge_equals_numpy_and_refuses_bad_indices(dev):
    from clibd_amd import ops

    rs = np.random.RandomState(5)
    for Q, m, T in ((1, 1, 257), (777, 5, 1000), (3001, 8, 257)):
        conf, idx_a, idx_b, la, lb, ql, thr = make_case(rs, Q, m, T)
        d = [torch.from_numpy(a).to(dev) for a in (conf, idx_a, idx_b)]
        for t in (thr[0], thr[len(thr) // 3], thr[-1]):
            merged, from_a = ops.threshold_merge(*d, la.shape[0], lb.shape[0], t)
            with np.errstate(invalid="ignore"):
                sel = conf.astype(np.float64) > t
            assert np.array_equal(merged.cpu().numpy(), np.where(sel, idx_a, la.shape[0] + idx_b))
            assert np.array_equal(from_a.cpu().numpy(), (sel * (1 << np.arange(m))[None, :]).sum(axis=1).astype(np.int32))
    conf, idx_a, idx_b, la, lb, ql, thr = make_case(rs, 100, 5, 257)
    seg = np.zeros(100, np.int32)
    for which, bad in ((1, la.shape[0]), (1, -1), (2, lb.shape[0]), (2, -7)):
        case = [conf, idx_a.copy(), idx_b.copy(), la, lb, ql, thr]
        case[which][37, 2] = bad
        d = [torch.from_numpy(a).to(dev) for a in case[:3]]
        with pytest.raises(ValueError, match="outside"):
            ops.threshold_merge(*d, la.shape[0], lb.shape[0], 0.5)
        with pytest.raises(ValueError, match="outside"):
            run_sweep(dev, case, seg, 1, [1, 3, 5])
    q2 = ql.copy()
    q2[5, 1] = -1
    with pytest.raises(ValueError, match="negative query label"):
        run_sweep(dev, [conf, idx_a, idx_b, la, lb, q2, thr], seg, 1, [1, 3, 5])
    with pytest.raises(ValueError, match="segment"):
        run_sweep(dev, [conf, idx_a, idx_b, la, lb, ql, thr], np.full(100, 2, np.int32), 2, [1, 3, 5])


def test_sweep_is_consistent_with_merge_and_label_hits(dev):
    from clibd_amd import ops

    rs = np.random.RandomState(8)
    Q, m, T, k_list = 5000, 5, 1000, [1, 3, 5]
    conf, idx_a, idx_b, la, lb, ql, thr = make_case(rs, Q, m, T)
    seg = segments(rs, Q, 2, True)
    sweep = run_sweep(dev, (conf, idx_a, idx_b, la, lb, ql, thr), seg, 2, k_list).cpu().numpy()
    d = [torch.from_numpy(a).to(dev) for a in (conf, idx_a, idx_b)]
    table = torch.from_numpy(np.concatenate([la, lb])).to(dev)
    n = np.maximum(np.concatenate([la, lb]).max(axis=0), ql.max(axis=0)) + 1
    off = [0] + np.cumsum(n).tolist()
    for t in (0, 1, 333, 500, 998, 999):
        merged, _ = ops.threshold_merge(*d, la.shape[0], lb.shape[0], thr[t])
        _, lh, _, _ = ops.topk_label_hits(merged, table, torch.from_numpy(ql).to(dev), off, k_list, segment=torch.from_numpy(seg).to(dev), nseg=2)
        assert np.array_equal(lh.cpu().numpy(), sweep[t]), t


# ------------------------------------------------------------------------------------------------------------ against the reference
def golden_lists(g, gen):
    """the list convention's inputs of both splits, from the reference's recorded searches"""
    sp = g["species"]
    lab_a = gen.labels_of(sp["seen_keys"])
    lab_b = gen.labels_of(np.concatenate([sp["val_unseen_keys"], sp["test_unseen_keys"]]))
    out = {}
    for split, qname in (("seen", "seen_query"), ("unseen", "unseen_query")):
        s = g["search"][split]
        pa = [{lv: [lab_a[i][lv] for i in row] for lv in LEVELS} for row in s["idx_a"]]
        pb = [{lv: [lab_b[i][lv] for i in row] for lv in LEVELS} for row in s["idx_b"]]
        out[split] = (pa, s["sim_a"].tolist(), pb, gen.labels_of(sp[qname]))
    return out


def codes_of(pred_list, g):
    vocab = [{x: i for i, x in enumerate(v)} for v in g["vocab"]]
    return np.array([[[vocab[l][x] for x in p[lv]] for l, lv in enumerate(LEVELS)] for p in pred_list])


def check_out(got, want, g, gt):
    assert got["micro_acc"] == want["micro_acc"]
    assert got["macro_acc"] == want["macro_acc"]
    assert got["per_class_acc"] == want["per_class_acc"]
    for k in g["k_list"]:
        for lv in LEVELS:
            assert list(got["per_class_acc"][k][lv]) == list(want["per_class_acc"][k][lv])       # same key order
    assert got["best_threshold"] == want["best_threshold"]
    assert got["gt_labels"] == gt
    assert np.array_equal(codes_of(got["final_pred_labels"], g), want["final_pred_codes"])


@pytest.mark.parametrize("name", ["small", "large"])
def test_list_convention_equals_reference(dev, golden, name):
    from clibd_amd import method_nn as M

    gen = _gen()
    g = golden[name]
    lists = golden_lists(g, gen)
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=g["k_list"]))
    ref_names = ("pred_labels_from_search_with_seen_keys", "pred_similarity_from_search_with_seen_keys", "pred_labels_from_search_with_unseen_keys", "gt_label")
    alt_names = ("pred_labels_from_a", "pred_confidence_from_a", "pred_labels_from_b", "gt_labels")
    splits = [dict(zip(ref_names, lists["seen"])), dict(zip(alt_names, lists["unseen"]))]                # both spellings
    for n in (1000, 1001):
        grid = np.linspace(0, 1, n)
        assert np.array_equal(M.sweep_top1_hits(splits, grid), g["hits"][n]), n
    assert M.search_threshold_with_harmonic_mean(args, splits) == g["best"][1000]
    assert M.search_threshold_with_harmonic_mean(None, splits, thresholds=np.linspace(0, 1, 1001), k_list=[1, 3, 5]) == g["best"][1001]
    assert M.search_threshold_with_harmonic_mean(args, splits, num_intervals=1001) == g["best"][1001]
    for split in ("seen", "unseen"):
        pa, sim, pb, gt = lists[split]
        check_out(M.get_final_pred_and_acc(args, pa, sim, pb, gt, best_threshold=g["best"][1000]), g["out"][split], g, gt)
        check_out(M.get_final_pred_and_acc(None, pa, sim, pb, gt, best_threshold=g["given_threshold"], k_list=g["k_list"]), g["out_at"][split], g, gt)
    pa, sim, pb, gt = lists["seen"]
    for thr, want in g["decide"].items():
        assert np.array_equal(codes_of(M.decide_prediction_with_threshold(args, pa, sim, pb, thr), g), want), thr
        final, gt2 = M.make_final_pred(args, pa, sim, pb, gt, thr)
        assert gt2 is gt and np.array_equal(codes_of(final, g), want)


def golden_features(g, gen, dev):
    f = {s: gen.synth(g["cfg"], s, g["redraw"].get(s)) for s in gen.SPLITS}
    sp = g["species"]
    t = lambda a: torch.from_numpy(a).to(dev)
    return dict(seen_query=t(f["seen_query"][0]), unseen_query=t(f["unseen_query"][0]), seen_keys=t(f["seen_keys"][0]),
                seen_keys_label=gen.labels_of(sp["seen_keys"]),
                unseen_keys=t(np.concatenate([f["val_unseen_keys"][1], f["test_unseen_keys"][1]])),
                unseen_keys_label=gen.labels_of(np.concatenate([sp["val_unseen_keys"], sp["test_unseen_keys"]])),
                seen_gt=gen.labels_of(sp["seen_query"]), unseen_gt=gen.labels_of(sp["unseen_query"]))


@pytest.mark.parametrize("name", ["small", "large"])
def test_features_convention_equals_reference(dev, golden, name):
    from clibd_amd import method_nn as M

    gen = _gen()
    g = golden[name]
    f = golden_features(g, gen, dev)
    if name == "large":
        assert f["seen_keys"].shape[0] >= 4096                                  # the pre-filtered search
    seen, unseen = M.seen_unseen_from_features(**f, k_list=g["k_list"])
    check_out(seen, g["out"]["seen"], g, f["seen_gt"])
    check_out(unseen, g["out"]["unseen"], g, f["unseen_gt"])
    seen1, unseen1 = M.seen_unseen_from_features(**f, k_list=g["k_list"], thresholds=np.linspace(0, 1, 1001))
    assert seen1["best_threshold"] == unseen1["best_threshold"] == g["best"][1001]
    # searched_threshold= is passed through (no search), and the index-array form agrees with the reference's searches
    seen2, unseen2 = M.seen_unseen_from_features(**f, k_list=g["k_list"], searched_threshold=g["given_threshold"])
    check_out(seen2, g["out_at"]["seen"], g, f["seen_gt"])
    check_out(unseen2, g["out_at"]["unseen"], g, f["unseen_gt"])
    seen3, _ = M.seen_unseen_from_features(**f, k_list=g["k_list"], searched_threshold=g["given_threshold"], with_predictions=False)
    s = g["search"]["seen"]
    want = np.where(s["sim_a"].astype(np.float64) > g["given_threshold"], s["idx_a"].astype(np.int64), len(f["seen_keys_label"]) + s["idx_b"].astype(np.int64))
    assert seen3["final_pred_labels"].dtype == np.int64 and np.array_equal(seen3["final_pred_labels"], want)
    assert seen3["micro_acc"] == seen2["micro_acc"]


# --------------------------------------------------------------------------------------------------------- a tiny model end to end
def test_method_1_agrees_with_features_entry_point(dev, capsys):
    from clibd_amd import eval as E
    from clibd_amd import method_nn as M

    from tests.test_eval_accuracy_gpu import loader, tiny_model

    model = tiny_model(dev)
    seen_q, unseen_q, seen_k, val_k, test_k = loader(11, 2), loader(12, 2), loader(13, 3), loader(14, 2), loader(15, 1)
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=[1, 3, 5]))
    seen, unseen = M.method_1_inference_and_eval_for_seen_and_unseen(args, model, seen_q, unseen_q, seen_k, val_k, test_k, dev)
    emb = [E.get_feature_and_label(dl, model, dev, as_numpy=False) for dl in (seen_q, unseen_q, seen_k, val_k, test_k)]
    want = M.seen_unseen_from_features(emb[0][1], emb[1][1], emb[2][1], emb[2][4], torch.cat([emb[3][2], emb[4][2]]), emb[3][4] + emb[4][4],
                                       emb[0][4], emb[1][4], [1, 3, 5])
    assert seen == want[0] and unseen == want[1]
    assert len(seen["final_pred_labels"]) == 16 and len(seen["final_pred_labels"][0]["species"]) == 5
    assert 0.0 <= seen["best_threshold"] <= 1.0
    # the reference's list-returning search, and its reporting helpers on the result
    sp, ss, sg, up, us, ug = M.inference_with_original_image_encoder_and_dna_encoder(model, seen_q, unseen_q, [val_k, test_k], dev, key_type="dna")
    assert len(sp) == 16 and ss.shape == (16, 5) and sg == emb[0][4] and len(up) == 16 and ug == emb[1][4]
    fixed = M.method_1_inference_and_eval_for_seen_and_unseen(args, model, seen_q, unseen_q, seen_k, val_k, test_k, dev, searched_threshold=0.125)
    assert fixed[0]["best_threshold"] == 0.125
    capsys.readouterr()
    M.print_acc_for_google_doc(seen, unseen)
    rows = capsys.readouterr().out.strip().splitlines()
    assert len(rows) == 6 and all(len(r.split()) == 12 for r in rows)
    species = sorted({d["species"] for d in emb[2][4]})
    frac = M.check_for_acc_about_correct_predict_seen_or_unseen(seen["final_pred_labels"], species)
    for k in (1, 3, 5):
        assert frac[k] == sum(any(s in species for s in r["species"][:k]) for r in seen["final_pred_labels"]) * 1.0 / 16


def test_all_zero_split_and_k_list_without_one(dev):
    from clibd_amd import method_nn as M

    gt = [{"order": "o0", "family": "f0", "genus": "g0", "species": "s0"}] * 6
    wrong = [{"order": ["o0"] * 3, "family": ["f0"] * 3, "genus": ["g0"] * 3, "species": ["s1", "s2", "s3"]}] * 6
    right = [{"order": ["o0"] * 3, "family": ["f0"] * 3, "genus": ["g0"] * 3, "species": ["s0", "s2", "s3"]}] * 6
    sim = [[0.875, 0.5, 0.125]] * 6                      # fp32 values, as a search returns them
    hopeless = {"pred_labels_from_a": wrong, "pred_confidence_from_a": sim, "pred_labels_from_b": wrong, "gt_labels": gt}
    fine = {"pred_labels_from_a": right, "pred_confidence_from_a": sim, "pred_labels_from_b": wrong, "gt_labels": gt}
    grid = np.linspace(0.25, 0.75, 11)
    assert M.search_threshold_with_harmonic_mean(None, [fine, hopeless], thresholds=grid, k_list=[1, 3]) == grid[0]     # the curve is 0 everywhere
    assert M.search_threshold_with_harmonic_mean(None, [fine, fine], k_list=[1, 3]) == 0.0                              # a plateau keeps its first threshold
    with pytest.raises(ValueError, match="must contain 1"):
        M.search_threshold_with_harmonic_mean(None, [fine], k_list=[3])
    with pytest.raises(ValueError, match="must contain 1"):
        M.seen_unseen_from_features(torch.zeros(2, 64, device=dev), torch.zeros(2, 64, device=dev), torch.zeros(9, 64, device=dev), gt[:1] * 9,
                                    torch.zeros(9, 64, device=dev), gt[:1] * 9, gt[:2], gt[:2], [3, 5])
    with pytest.raises(ValueError, match="not an fp32 value"):
        M.decide_prediction_with_threshold(None, right, [[0.1, 0.2, 0.3]] * 6, wrong, 0.5)
