"""CPU checks of the embedding analysis: the fifth header (include/clibd_hip_analysis.h) and its binding table, host-side validation of the
C entries, the unit's register report, the planning helpers, the stated divergences that raise, and the fixture
(tests/golden/analysis_golden.pt, made by tests/golden/make_analysis_golden.py) against the numpy restatement of tests/analysis_reference.py."""
import ctypes
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import analysis_reference as AR  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_analysis.h"
LEVELS = ["order", "family", "genus", "species"]
SYMBOLS = ["clibd_confusion_counts", "clibd_same_label_nearest", "clibd_silhouette_samples", "clibd_silhouette_workspace_bytes"]


def gen_module():
    spec = importlib.util.spec_from_file_location("make_analysis_golden", ROOT / "tests" / "golden" / "make_analysis_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "analysis_golden.pt", weights_only=False)


@pytest.fixture(scope="module")
def world(golden):
    G = gen_module()
    return G, G.make_dicts(golden["cfg"], golden["redraw"])


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_analysis_header_symbols_opening_comment_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert "analysis" in build.SOURCES and HEADER in build._deps()


def test_analysis_unit_uses_no_scratch():
    """the compiler remark that test_hot_kernels_use_no_scratch reads: every kernel of analysis.hip keeps its working set in registers"""
    from clibd_amd import build

    out = [(k["name"], k["scratch"]) for k in build.resource_usage("analysis")]
    assert len(out) == 7 and any("silhouette_tile_kernel" in n for n, _ in out), out
    assert not [(n, s) for n, s in out if s != 0], out


def test_analysis_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    N, D, C = 300, 64, 5
    need = L.clibd_silhouette_workspace_bytes(N, 0)
    assert need % 16 == 0 and need >= 8 * N + 16 * N
    assert L.clibd_silhouette_workspace_bytes(N, 64) >= 8 * N + 16 * N * 5 > need
    assert L.clibd_silhouette_workspace_bytes(0, 0) == 0 and L.clibd_silhouette_workspace_bytes(N, 100) == 0
    assert L.clibd_silhouette_workspace_bytes(N, -64) == 0
    a, b, c, ws = P(1 << 12), P(1 << 13), P(1 << 14), P(1 << 20)
    good = np.array([0, 10, 11, 200, 250, 300], dtype=np.int32)

    def sil(X=a, N=N, D=D, seg=b, host=good, C=C, chunk=0, s=c, ws=ws, nbytes=need):
        hp = None if host is None else host.ctypes.data_as(P)
        return L.clibd_silhouette_samples(X, N, D, seg, hp, C, chunk, s, ws, nbytes, None)

    two = np.array([0, 1, 2], dtype=np.int32)
    for kw, word in ((dict(X=None), b"null"), (dict(seg=None), b"null"), (dict(host=None), b"null"), (dict(s=None), b"null"), (dict(ws=None), b"null"),
                     (dict(N=2, C=2, host=two), b"N must be"), (dict(C=1, host=np.array([0, 300], dtype=np.int32)), b"2 to n_samples - 1"),
                     (dict(N=3, C=3, host=np.array([0, 1, 2, 3], dtype=np.int32)), b"2 to n_samples - 1"),
                     (dict(host=np.array([0, 10, 200, 11, 250, 300], dtype=np.int32)), b"seg must rise"),
                     (dict(host=np.array([0, 10, 10, 200, 250, 300], dtype=np.int32)), b"seg must rise"),
                     (dict(host=np.array([1, 10, 11, 200, 250, 300], dtype=np.int32)), b"seg must rise"),
                     (dict(host=np.array([0, 10, 11, 200, 250, 299], dtype=np.int32)), b"seg must rise"),
                     (dict(D=100), b"multiple of 32"), (dict(D=0), b"multiple of 32"), (dict(chunk=100), b"col_chunk"), (dict(chunk=-64), b"col_chunk"),
                     (dict(X=P((1 << 12) + 4)), b"aligned"), (dict(nbytes=need - 1), b"clibd_silhouette_workspace_bytes"),
                     (dict(chunk=64), b"clibd_silhouette_workspace_bytes"), (dict(ws=P((1 << 20) + 8)), b"misaligned")):
        assert sil(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())

    kseg = np.array([0, 4, 4, 9], dtype=np.int32)     # an empty class is allowed here

    def near(Q=a, ldq=D, K=b, ldk=D, Nq=7, Nk=9, D=D, seg=c, host=kseg, C=3, qc=ws, dist=a, arg=b):
        hp = None if host is None else host.ctypes.data_as(P)
        return L.clibd_same_label_nearest(Q, ldq, K, ldk, Nq, Nk, D, seg, hp, C, qc, dist, arg, None)

    for kw, word in ((dict(Q=None), b"null"), (dict(K=None), b"null"), (dict(seg=None), b"null"), (dict(host=None), b"null"), (dict(qc=None), b"null"),
                     (dict(dist=None), b"null"), (dict(arg=None), b"null"), (dict(Nq=0), b"non-positive"), (dict(D=0), b"non-positive"),
                     (dict(ldq=D - 1), b"ldq and ldk"), (dict(ldk=D - 1), b"ldq and ldk"), (dict(host=np.array([0, 5, 4, 9], dtype=np.int32)), b"seg must rise"),
                     (dict(host=np.array([0, 4, 4, 8], dtype=np.int32)), b"seg must rise")):
        assert near(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())

    def conf(t=a, p=b, N=10, C=4, out=c):
        return L.clibd_confusion_counts(t, p, N, C, out, None)

    for kw, word in ((dict(t=None), b"null"), (dict(p=None), b"null"), (dict(out=None), b"null"), (dict(N=0), b"non-positive"), (dict(C=0), b"non-positive"),
                     (dict(C=46341), b"too large")):
        assert conf(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())


# ---- planning -------------------------------------------------------------------------------------------------------------------------
def test_sort_permutation_segments_and_chunks():
    from clibd_amd import analysis as A

    codes = np.array([7, 3, 7, 7, 11, 3, 7], dtype=np.int64)
    order, seg = A.plan_clusters(codes)
    assert order.tolist() == [1, 5, 0, 2, 3, 6, 4] and seg.tolist() == [0, 2, 6, 7] and seg.dtype == np.int32
    assert (np.diff(codes[order]) >= 0).all()
    order_t, seg_t = A.plan_clusters(torch.from_numpy(codes))
    assert order_t.tolist() == order.tolist() and seg_t.tolist() == seg.tolist()
    rs = np.random.RandomState(0)
    codes = rs.randint(0, 40, 500) * 3
    order, seg = A.plan_clusters(codes)
    assert sorted(order.tolist()) == list(range(500)) and seg[0] == 0 and seg[-1] == 500 and (np.diff(seg) > 0).all()
    for c in range(len(seg) - 1):
        run = order[seg[c]:seg[c + 1]]
        assert len(set(codes[run].tolist())) == 1 and (np.diff(run) > 0).all()          # one cluster per run, stable inside it
    with pytest.raises(ValueError):
        A.plan_clusters(np.zeros((2, 2), dtype=np.int64))
    order, seg = A.plan_groups(np.array([2, 0, 2, 4]), 6)
    assert order.tolist() == [1, 0, 2, 3] and seg.tolist() == [0, 1, 1, 3, 3, 4, 4]
    assert A.chunk_plan(257, 64) == [(0, 64), (64, 128), (128, 192), (192, 256), (256, 257)]
    assert A.chunk_plan(257) == [(0, 257)] and A.chunk_plan(2049) == [(0, 1024), (1024, 2048), (2048, 2049)]
    for bad in (100, -64):
        with pytest.raises(ValueError):
            A.chunk_plan(257, bad)
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    assert A.pad_width(x, 4) is x
    p = A.pad_width(torch.ones(3, 100))
    assert p.shape == (3, 128) and float(p[:, :100].min()) == 1 and float(p[:, 100:].abs().max()) == 0
    assert A.BINS == [0.0, 0.3, 0.6, 0.9, 1.2, 1.5] and A.K_STEP == 32


def test_chunk_bookkeeping_restatement_equals_the_direct_form():
    """head / tail / fold and the stitch in order give the silhouette for every chunk width, a dominant cluster crossing many chunks,
    singletons at chunk borders, C = 2 and C = N - 1"""
    rs = np.random.RandomState(3)
    for N, C, cc in ((130, 4, 64), (257, 7, 64), (200, 127, 64), (150, 2, 64), (100, 99, 64), (257, 7, 128), (129, 5, 1024)):
        X = rs.randn(N, 8)
        if C == N - 1:
            codes = np.arange(N)
            codes[-1] = 0
        else:
            codes = np.where(rs.rand(N) < 0.8, 0, rs.randint(0, C, N))
            codes[:C] = np.arange(C)
        order = np.argsort(codes, kind="stable")
        seg = np.concatenate([[0], np.cumsum(np.unique(codes, return_counts=True)[1])])
        direct = AR.silhouette_fp64(X, codes)
        chunked = np.empty(N)
        chunked[order] = AR.silhouette_chunked(X[order], seg, cc)
        assert np.abs(direct - chunked).max() < 1e-13, (N, C, cc)


# ---- the fixture against the restatement ------------------------------------------------------------------------------------------------
def test_golden_silhouette_agrees_with_the_restatement(golden, world):
    G, (keys_dict, _, _) = world
    X = keys_dict["encoded_image_feature"]
    assert X.dtype == np.float32 and X.shape == (300, 64)
    assert np.abs(np.sqrt((X.astype(np.float64) ** 2).sum(axis=1)) - 1).max() < 1e-6
    codes = G_codes(keys_dict["label_list"])
    for l, lv in enumerate(LEVELS):
        ref = golden["sil"][lv]
        assert ref.dtype == np.float32 and ref.shape == (300,)
        s64 = AR.silhouette_fp64(X, codes[:, l])
        err = np.abs(s64 - ref.astype(np.float64)).max()
        print(f"{lv}: sklearn fp32 vs fp64 restatement {err:.3e}")
        assert err <= 5e-7
        emu = np.abs(s64 - AR.silhouette_fp32_gram(X, codes[:, l]).astype(np.float64)).max()
        print(f"{lv}: fp32 Gram emulation vs fp64 {emu:.3e}")
        assert emu < 5e-6
        assert abs(golden["sil_printed"][lv] - float(ref.astype(np.float64).mean())) < 2e-6
        counts = np.unique(codes[:, l], return_counts=True)[1]
        assert counts.min() == 1 and (s64[counts[codes[:, l]] == 1] == 0).all()
        if lv == "order":
            assert counts.max() >= 0.8 * len(X)
    d = np.sqrt(np.maximum(2 - 2 * X.astype(np.float64) @ X.astype(np.float64).T, 0))
    np.fill_diagonal(d, np.inf)
    assert d.min() >= 0.5
    nested = {l["genus"] for l in keys_dict["label_list"] if l["species"] == "not_classified"}
    assert len(nested) >= 3


def G_codes(label_list):
    from clibd_amd.eval import LabelCodec

    return LabelCodec().encode(label_list)


def test_golden_distances_histogram_and_confusion_agree_with_the_restatement(golden, world):
    from clibd_amd import analysis as A

    G, (keys_dict, seen_dict, unseen_dict) = world
    klab = [l["species"] for l in keys_dict["label_list"]]
    edges = np.array(golden["bins"])
    cols = {}
    for split, qd in (("seen", seen_dict), ("unseen", unseen_dict)):
        qlab = [l["species"] for l in qd["label_list"]]
        assert set(qlab) <= set(klab)
        assert len(golden["dist"][split]) == 9
        for qf in G.FEATURES:
            for kf in G.FEATURES:
                ref = golden["dist"][split][f"{qf}_{kf}"]
                d, arg, _ = AR.nearest_fp64(qd[qf], keys_dict[kf], qlab, klab)
                np.testing.assert_allclose(d, ref, rtol=1e-12, atol=0)
                assert (np.array(klab)[arg] == np.array(qlab)).all()
                assert np.abs(ref[:, None] - edges[None, :]).min() >= golden["edge_gap"] == 1e-3
                cols[(split, qf, kf)] = ref
    img, dna, lang = G.FEATURES
    series = {"Image-to-Image": (img, img), "DNA-to-DNA": (dna, dna), "Image-to-DNA": (img, dna), "Image-to-Text": (dna, lang)}   # the reference's column
    for name, (qf, kf) in series.items():
        both = np.concatenate([cols[("seen", qf, kf)], cols[("unseen", qf, kf)]])
        assert np.array_equal(A.distance_histogram(both), golden["hist"][name])
        assert golden["hist"][name].sum() == len(both)
    head = golden["records_head"][0]
    assert list(head) == ["file_name", "order", "family", "genus", "species", "distance_for_image_to_image", "distance_for_dna_to_dna",
                          "distance_for_image_to_dna", "distance_for_dna_to_image", "distance_for_image_to_language", "split"]
    assert head["file_name"] == "seen0" and head["split"] == "val_seen"
    assert head["distance_for_image_to_language"] == cols[("seen", dna, lang)][0] != cols[("seen", img, lang)][0]
    # confusion: counts under ==, and the host selections of the module on the recorded counts
    sizes = set()
    for (split, q, k, lv), c in golden["confusion"].items():
        qd = seen_dict if split == "seen" else unseen_dict
        classes = sorted({g[lv] for g in qd["label_list"]})
        assert classes == c["labels"]
        m = {x: i for i, x in enumerate(classes)}
        t = np.array([m[g[lv]] for g in qd["label_list"]])
        p = np.array([m.get(keys_dict["label_list"][int(j)][lv], -1) for j in golden["idx"][split][(q, k)]])
        cm = AR.confusion_np(t, p, len(classes))
        assert np.array_equal(cm, c["cm"])
        assert not G.selection_ties(cm)
        sizes.add(len(classes))
        for name, fn in (("largest", A._largest_10), ("most_confused", A._most_confused_10)):
            sub, labels = fn(cm, classes)
            assert labels == c[name][1] and np.array_equal(sub, c[name][0]), (split, q, k, lv, name)
    assert len(golden["confusion"]) == 24 and max(sizes) > 10 and min(sizes) < 10


def test_normalisation_and_stable_selections():
    from clibd_amd import analysis as A

    cm = np.array([[2, 1, 0], [0, 0, 0], [1, 1, 2]])
    n = A.normalized_confusion(cm)
    assert np.array_equal(n, np.array([[2 / 3, 1 / 3, 0], [0, 0, 0], [0.25, 0.25, 0.5]]))
    sub, labels = A._largest_10(cm, ["a", "b", "c"])
    assert labels == ["a", "c", "b"]                                # equal counts keep class order
    assert np.array_equal(sub, n[np.ix_([0, 2, 1], [0, 2, 1])])
    big = np.eye(12, dtype=np.int64) * 5
    big[3, 7] = 4
    big[9, 2] = 3
    sub, labels = A._most_confused_10(big, list("abcdefghijkl"))
    assert len(labels) == 10 and {"d", "h", "j", "c"} <= set(labels) and labels == sorted(labels)


# ---- the module without a GPU -----------------------------------------------------------------------------------------------------------
def test_module_imports_and_divergences_raise_without_a_gpu(world):
    from clibd_amd import analysis as A

    for name in ("calculate_silhouette_score", "get_similarity_for_different_combination_of_modalities", "confusion_matrix", "normalized_confusion",
                 "largest_10_classes", "most_confused_10_classes", "silhouette_samples", "silhouette_by_level", "nearest_same_species",
                 "distance_histogram", "confusion_from_predictions"):
        assert callable(getattr(A, name)), name
    doc = A.__doc__
    for word in ("float64 mean", "sorted", "stable", "distance_for_image_to_language", "KeyError", "ValueError"):
        assert word in doc, word
    x = np.zeros((6, 8), dtype=np.float32)
    for codes in (np.zeros(6, dtype=np.int64), np.arange(6)):          # 1 cluster, N clusters
        with pytest.raises(ValueError, match="Valid values are 2 to n_samples - 1"):
            A.silhouette_samples(x, codes)
    with pytest.raises(ValueError, match="Valid values are 2 to n_samples - 1"):
        A.silhouette_by_level(x, [{"order": "o", "family": "f", "genus": "g", "species": f"s{i % 2}"} for i in range(6)])
    G, (keys_dict, seen_dict, unseen_dict) = world
    orphan = dict(seen_dict, label_list=[dict(seen_dict["label_list"][0], species="nobody")] + seen_dict["label_list"][1:])
    with pytest.raises(KeyError, match="nobody"):
        A.get_similarity_for_different_combination_of_modalities(keys_dict, orphan, unseen_dict, None)
    with pytest.raises(ValueError):
        A.confusion_matrix(["a"], ["a", "b"], ["a", "b"])
    pred = {"seen_gt_label": seen_dict["label_list"], "unseen_gt_label": unseen_dict["label_list"],
            "encoded_image_feature": {"encoded_image_feature": {"curr_seen_pred_list": np.zeros((226, 5), dtype=np.int64)}}}
    with pytest.raises(ValueError, match="keys_label"):
        A.confusion_from_predictions(pred, pairs=[("encoded_image_feature", "encoded_image_feature")])
