"""CPU checks of the eval phase: the host finaliser (integer counts -> the reference's float64 accuracy tables) against the reference's
recorded values (tests/golden/eval_golden.pt, tests/golden/make_eval_golden.py), the label codec, compute_overall_acc, and the host-side
validation of the new C entry points (no GPU needed)."""
import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "eval_golden.pt"
LEVELS = ["order", "family", "genus", "species"]


def _gen():
    spec = importlib.util.spec_from_file_location("make_eval_golden", ROOT / "tests" / "golden" / "make_eval_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def restated_counts(gt_ids, pred_ids, n_classes_per_level, k_list):
    """The hits kernel restated in numpy: gt_ids [Q, L], pred_ids [Q, L, m] (class ids of the predicted labels)."""
    Q, L, m = pred_ids.shape
    match = pred_ids == gt_ids[:, :, None]
    first = np.where(match.any(axis=2), match.argmax(axis=2), m)
    off = np.concatenate([[0], np.cumsum(n_classes_per_level)])
    C = int(off[-1])
    level_hits = np.stack([(first < k).sum(axis=0) for k in k_list]).astype(np.int32)
    cls = gt_ids + off[:-1][None, :]
    class_count = np.bincount(cls.ravel(), minlength=C).astype(np.int32)
    class_hits = np.stack([np.bincount(cls.ravel(), weights=(first < k).ravel(), minlength=C) for k in k_list]).astype(np.int32)
    return level_hits, class_hits, class_count, [int(v) for v in off]


def finalise(gt_labels, pred_lists, k_list):
    """labels -> codec ids -> restated integer counts -> eval._split_accuracy"""
    from clibd_amd.eval import LabelCodec, _split_accuracy

    codec = LabelCodec()
    gt = codec.encode(gt_labels)
    m = len(pred_lists[0][LEVELS[0]])
    pred = np.stack([codec.encode([{lv: p[lv][r] for lv in LEVELS} for p in pred_lists]) for r in range(m)], axis=2)
    lh, ch, cc, off = restated_counts(gt, pred, [len(mp) for mp in codec.maps], k_list)
    assert off == codec.class_offset()
    return _split_accuracy(lh, ch, cc, gt, codec, off, k_list, list(range(len(k_list))))


def test_finaliser_reproduces_reference_standalone(golden):
    g = golden["standalone"]
    gt = [{lv: f"{lv[0]}{g['gt'][q, l]}" for l, lv in enumerate(LEVELS)} for q in range(len(g["gt"]))]
    pr = [{lv: [f"{lv[0]}{x}" for x in g["preds"][q, l]] for l, lv in enumerate(LEVELS)} for q in range(len(g["gt"]))]
    micro, macro, per_class = finalise(gt, pr, g["k_list"])
    assert micro == g["micro"]
    assert macro == g["macro"]
    assert per_class == g["per_class"]
    for k in g["k_list"]:
        for lv in LEVELS:
            assert list(per_class[k][lv]) == list(g["per_class"][k][lv])     # the classes in order of first appearance


@pytest.mark.parametrize("name", ["small", "large"])
def test_finaliser_reproduces_reference_inference_tables(golden, name):
    gen = _gen()
    g = golden[name]
    vocab = g["vocab"]
    gt = {s: [gen.taxonomy(int(x)) for x in g["species"][s]] for s in ("seen", "unseen")}
    n = 0
    for (qt, kt), codes in g["pred_codes"].items():
        for split, c in zip(("seen", "unseen"), codes):
            preds = [{lv: [vocab[l][x] for x in c[q, l]] for l, lv in enumerate(LEVELS)} for q in range(c.shape[0])]
            micro, macro, per_class = finalise(gt[split], preds, g["k_list"])
            assert micro == g["acc_dict"][qt][kt][split]["micro_acc"], (qt, kt, split)
            assert macro == g["acc_dict"][qt][kt][split]["macro_acc"], (qt, kt, split)
            assert per_class == g["per_class_acc"][qt][kt][split], (qt, kt, split)
            n += 1
    assert n == 2 * 21      # 4 query types x 5 key types of width D, and concatenated x concatenated


def test_golden_is_what_the_generator_describes(golden):
    """the features the GPU tests regenerate are the ones the reference saw"""
    gen = _gen()
    for name in ("small", "large"):
        g = golden[name]
        for s in ("keys", "seen", "unseen"):
            assert gen.checksum(gen.synth_split(g["cfg"], s, g["redraw"].get(s))) == g["checksum"][s], (name, s)


def test_compute_overall_acc_matches_reference(golden):
    from clibd_amd.eval import compute_overall_acc

    for name in ("small", "large"):
        assert compute_overall_acc(golden[name]["acc_dict"]) == golden[name]["overall_acc"]


def test_label_codec_round_trips():
    from clibd_amd.eval import LabelCodec

    rs = np.random.RandomState(0)
    labels = [{"order": f"o{a}", "family": ("f", int(b)), "genus": int(c), "species": f"s{d}"} for a, b, c, d in rs.randint(0, 7, (500, 4))]
    codec = LabelCodec()
    ids = codec.encode(labels[:300])
    more = codec.encode(labels[300:])                   # a later split: known labels keep their ids, new ones are appended
    assert ids.dtype == np.int32 and ids.shape == (300, 4)
    assert codec.decode(ids) == labels[:300] and codec.decode(more) == labels[300:]
    assert np.array_equal(codec.encode(labels[:300]), ids)
    off = codec.class_offset()
    assert off[0] == 0 and [off[i + 1] - off[i] for i in range(4)] == [len(set(str(d[lv]) for d in labels)) for lv in LEVELS]
    for l in range(4):
        assert ids[:, l].max() < off[l + 1] - off[l]
    rows = codec.decode_rows(ids, np.array([[3, 1], [0, 0]]))
    assert rows[0] == {lv: [labels[3][lv], labels[1][lv]] for lv in LEVELS}


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _arr(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _hits(L, Q=10, kmax=5, Nk=20, nl=4, off=(0, 2, 4, 6, 8), ks=(1, 3, 5), seg=None, nseg=1):
    P = ctypes.c_void_p(256)
    return L.clibd_topk_label_hits(P, Q, kmax, P, Nk, P, nl, None if off is None else _arr(off), _arr(ks), len(ks), seg, nseg, P, P, P, P, P, None)


def test_label_hits_validation_needs_no_gpu(lib):
    L = lib
    assert _hits(L, Q=0) == -1 and b"Q > 0" in L.clibd_last_error()
    assert _hits(L, Nk=0) == -1
    assert _hits(L, nl=9, off=tuple(range(10))) == -1
    assert _hits(L, kmax=9) == -1 and b"kmax" in L.clibd_last_error()
    assert _hits(L, ks=(1, 3, 6)) == -1 and b"k <= kmax" in L.clibd_last_error()             # k > kmax
    assert _hits(L, ks=(1, 5, 3)) == -1 and b"ascending" in L.clibd_last_error()
    assert _hits(L, ks=(1, 1)) == -1 and b"ascending" in L.clibd_last_error()
    assert _hits(L, ks=tuple(range(1, 10)), kmax=8) == -1
    assert _hits(L, off=None) == -1 and b"null" in L.clibd_last_error()
    assert _hits(L, off=(1, 2, 4, 6, 8)) == -1
    assert _hits(L, off=(0, 2, 1, 6, 8)) == -1 and b"non-decreasing" in L.clibd_last_error()
    assert _hits(L, nseg=2) == -1 and b"nseg" in L.clibd_last_error()                        # two segments need a segment array
    P = ctypes.c_void_p(256)
    assert L.clibd_topk_label_hits(None, 10, 5, P, 20, P, 4, _arr((0, 2, 4, 6, 8)), _arr((1,)), 1, None, 1, P, P, P, P, P, None) == -1
    assert L.clibd_topk_label_hits(P, 10, 5, P, 20, P, 4, _arr((0, 2, 4, 6, 8)), None, 1, None, 1, P, P, P, P, P, None) == -1


def test_pair_features_validation_needs_no_gpu(lib):
    P = ctypes.c_void_p(256)
    assert lib.clibd_eval_pair_features(None, P, 4, 8, P, P, None) == -1
    assert lib.clibd_eval_pair_features(P, P, 4, 6, P, P, None) == -1 and b"multiple of 4" in lib.clibd_last_error()
    assert lib.clibd_eval_pair_features(P, P, 0, 8, P, P, None) == -1
    assert lib.clibd_eval_pair_features(P, ctypes.c_void_p(260), 4, 8, P, P, None) == -1 and b"alignment" in lib.clibd_last_error()


def test_wrappers_refuse_host_tensors():
    from clibd_amd import ops

    with pytest.raises(ValueError):
        ops.topk_label_hits(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32),
                            [0, 1, 2, 3, 4], [1])
    with pytest.raises(ValueError):
        ops.eval_pair_features(torch.zeros(2, 8), torch.zeros(2, 8))
