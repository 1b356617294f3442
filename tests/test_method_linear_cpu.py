"""CPU checks of the linear-probe classifier: the fourth header (include/clibd_hip_classifier.h) and its binding table, host-side
validation of the C entries, the module's import, and the fixture (tests/golden/method_linear_golden.pt, made by
tests/golden/make_method_linear_golden.py) against an fp64 restatement of the head, the cross-entropy and the softmax top-k written here,
the host helpers and the 1 001-point grid."""
import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "clibd_hip_classifier.h"
LEVELS = ["order", "family", "genus", "species"]
SYMBOLS = ["clibd_ce_rows_bwd", "clibd_ce_rows_fwd", "clibd_ce_rows_workspace_bytes", "clibd_linear_f32_bwd", "clibd_linear_f32_fwd",
           "clibd_linear_f32_workspace_bytes", "clibd_softmax_topk"]


def _gen():
    spec = importlib.util.spec_from_file_location("make_method_linear_golden", ROOT / "tests" / "golden" / "make_method_linear_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "method_linear_golden.pt", weights_only=False)


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_classifier_header_symbols_and_shared_split_kernels():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert HEADER in build._deps() and "classifier" in build.SOURCES
    # the split-image kernels are shared through a header, not copied
    assert "split3.h" in (build.CSRC / "loss.hip").read_text() and "split3.h" in (build.CSRC / "classifier.hip").read_text()
    assert "void split3_kernel" not in (build.CSRC / "loss.hip").read_text() + (build.CSRC / "classifier.hip").read_text()


def test_classifier_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    B, C, D = 33, 916, 768
    need = L.clibd_linear_f32_workspace_bytes(B, C, D)
    assert need % 16 == 0 and need >= (B + 928) * 3 * D * 2 + B * 928 * 4
    assert L.clibd_linear_f32_workspace_bytes(0, C, D) == 0 and L.clibd_linear_f32_workspace_bytes(B, -1, D) == 0
    assert L.clibd_linear_f32_workspace_bytes(257, C, D) > need
    a, b, c, d, e, ws = P(1 << 12), P(1 << 13), P(1 << 14), P(1 << 15), P(1 << 16), P(1 << 20)

    def fwd(x=a, w=b, bias=c, B=B, C=C, D=D, out=d, ld=C, ws=ws, nbytes=need):
        return L.clibd_linear_f32_fwd(x, w, bias, B, C, D, out, ld, ws, nbytes, None)

    def bwd(dout=a, x=b, w=c, B=B, C=C, D=D, dx=d, dw=e, db=None, ws=ws, nbytes=need):
        return L.clibd_linear_f32_bwd(dout, x, w, B, C, D, dx, dw, db, ws, nbytes, None)

    for fn in (fwd, bwd):
        for kw, word in ((dict(x=None), b"null"), (dict(w=None), b"null"), (dict(ws=None), b"null"), (dict(D=100), b"multiple of 64"),
                         (dict(D=0), b"non-positive"), (dict(B=0), b"non-positive"), (dict(C=-4), b"non-positive"),
                         (dict(nbytes=need - 1), b"clibd_linear_f32_workspace_bytes"), (dict(nbytes=0), b"clibd_linear_f32_workspace_bytes"),
                         (dict(ws=P((1 << 20) + 8)), b"misaligned"), (dict(x=P((1 << 12) + 4)), b"aligned")):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert word in L.clibd_last_error(), (fn.__name__, kw, L.clibd_last_error())
    assert fwd(out=None) == -1 and b"null" in L.clibd_last_error()
    assert fwd(ld=C - 1) == -1 and b"ld_out" in L.clibd_last_error()
    assert bwd(dout=None) == -1 and b"null" in L.clibd_last_error()
    assert bwd(dx=P((1 << 15) + 4)) == -1 and b"aligned" in L.clibd_last_error()

    need_ce = L.clibd_ce_rows_workspace_bytes(B)
    assert need_ce >= 4 * B and need_ce % 16 == 0 and L.clibd_ce_rows_workspace_bytes(0) == 0

    def ce_fwd(logits=a, ld=C, target=b, B=B, C=C, lse=c, loss=d, err=e, ws=ws, nbytes=need_ce):
        return L.clibd_ce_rows_fwd(logits, ld, target, B, C, lse, loss, err, ws, nbytes, None)

    for kw, word in ((dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(lse=None), b"null"), (dict(loss=None), b"null"),
                     (dict(ws=None), b"null"), (dict(ld=C - 1), b"ld must"), (dict(B=0), b"non-positive"), (dict(C=0), b"non-positive"),
                     (dict(nbytes=need_ce - 1), b"clibd_ce_rows_workspace_bytes"), (dict(ws=P((1 << 20) + 4)), b"misaligned")):
        assert ce_fwd(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())

    def ce_bwd(logits=a, ld=C, target=b, lse=c, B=B, C=C, dloss=None, d=d, ld_d=C):
        return L.clibd_ce_rows_bwd(logits, ld, target, lse, B, C, dloss, d, ld_d, None)

    for kw, word in ((dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(lse=None), b"null"), (dict(d=None), b"null"),
                     (dict(ld=C - 1), b"ld must"), (dict(ld_d=C - 1), b"ld_d"), (dict(B=-1), b"non-positive")):
        assert ce_bwd(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())

    def topk(logits=a, ld=C, B=B, C=C, k=5, conf=b, idx=c):
        return L.clibd_softmax_topk(logits, ld, B, C, k, conf, idx, None)

    for kw, word in ((dict(logits=None), b"null"), (dict(conf=None), b"null"), (dict(idx=None), b"null"), (dict(k=0), b"1..8"), (dict(k=9), b"1..8"),
                     (dict(k=-1), b"1..8"), (dict(C=4, ld=4, k=5), b"out of range"), (dict(ld=C - 1), b"ld must"), (dict(B=0), b"non-positive")):
        assert topk(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())


def test_module_imports_without_a_gpu():
    from clibd_amd import method_linear as ML
    from clibd_amd import method_nn as NN
    from clibd_amd.engine import NotSupportedYet

    for name in ("ViTWIthExtraLayer", "CrossEntropyLoss", "build_image_classifier", "fine_tuning_epoch", "evaluate_epoch", "train_image_classifier",
                 "load_all_seen_species_name_and_create_label_map", "label_batch_to_species_idx", "get_all_unique_species_from_dataloader",
                 "inference_with_fine_tuned_image_encoder", "method_2_inference_and_eval_for_seen_and_unseen", "classifier_seen_unseen_from_features",
                 "search_threshold_with_harmonic_mean", "get_final_pred_and_acc", "decide_prediction_with_threshold", "make_final_pred"):
        assert callable(getattr(ML, name)), name
    assert ML.harmonic_mean is NN.harmonic_mean and ML.print_acc_for_google_doc is NN.print_acc_for_google_doc
    assert ML.check_for_acc_about_correct_predict_seen_or_unseen is NN.check_for_acc_about_correct_predict_seen_or_unseen
    for kw in (dict(weight=torch.ones(3)), dict(label_smoothing=0.1), dict(ignore_index=0), dict(reduction="sum")):
        with pytest.raises(NotSupportedYet):
            ML.CrossEntropyLoss(**kw)
    ML.CrossEntropyLoss()
    m = ML.ViTWIthExtraLayer(torch.nn.Identity(), torch.nn.Linear(128, 36))
    assert sorted(m.state_dict()) == ["new_linear_layer.bias", "new_linear_layer.weight"]
    m = ML.ViTWIthExtraLayer(torch.nn.Linear(8, 128), torch.nn.Linear(128, 36))
    assert sorted(m.state_dict()) == ["new_linear_layer.bias", "new_linear_layer.weight", "vit.bias", "vit.weight"]


# ---- the fixture against an fp64 restatement ----------------------------------------------------------------------------------------
def restated(x, w, b, t=None, k=5):
    """fp64: logits, confidences and indices of topk(softmax), and with targets the mean cross-entropy and its gradients"""
    x, w, b = (np.asarray(v, dtype=np.float64) for v in (x, w, b))
    logits = x @ w.T + b
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    idx = np.argsort(-p, axis=1, kind="stable")[:, :k]
    out = {"logits": logits, "conf": np.take_along_axis(p, idx, 1), "idx": idx}
    if t is not None:
        B = x.shape[0]
        out["loss"] = float(np.mean(-np.log(p[np.arange(B), t])))
        g = p.copy()
        g[np.arange(B), t] -= 1.0
        g /= B
        out.update(dx=g @ w, dw=g.T @ x, db=g.sum(axis=0))
    return out


def test_golden_agrees_with_the_fp64_restatement(golden):
    G = _gen()
    g = golden
    w, b = g["head"]["weight"], g["head"]["bias"]
    assert w.shape == (36, 128) and b.shape == (36,) and w.dtype == np.float32
    lin = G.head0()
    assert np.array_equal(lin.weight.detach().numpy(), g["head0"]["weight"]) and np.array_equal(lin.bias.detach().numpy(), g["head0"]["bias"])
    feats = {s: G.synth(s, g["redraw"][s])[0] for s in ("seen_query", "unseen_query")}
    # the kernel case
    k = g["kernel"]
    r = restated(feats["seen_query"][:33], w, b, k["target"])
    assert k["logits"].shape == (33, 36) and k["dw"].shape == (36, 128) and k["dx"].shape == (33, 128) and k["db"].shape == (36,)
    for name in ("logits", "dx", "dw", "db"):
        np.testing.assert_allclose(r[name], k[name], rtol=1e-12, atol=1e-14)
    assert abs(r["loss"] - k["loss"]) < 1e-13
    # the reference's fp32 confidences are the fp64 ones to fp32 accuracy, the indices equal, and every decision has its margin
    grid = np.linspace(0, 1, 1001)[1:-1]
    for s in ("seen_query", "unseen_query"):
        r = restated(feats[s], w, b, k=6)
        conf = g["conf"][s].astype(np.float64)
        assert conf.dtype == np.float64 and g["conf"][s].dtype == np.float32 and conf.shape == (len(feats[s]), 5)
        assert np.abs(conf - r["conf"][:, :5]).max() < 2e-6
        assert np.array_equal(g["idx"][s].astype(np.int64), r["idx"][:, :5])
        assert (conf > 0).all() and (conf <= 1).all()
        assert np.abs(conf[:, :, None] - grid[None, None, :]).min() > g["gap"] == 2e-5
        assert (r["conf"][:, :-1] - r["conf"][:, 1:]).min() > g["gap"] - 1e-6
    assert 0.3 <= g["median_top1"] <= 0.9 and g["mixed"] >= 20 and g["logits_absmax"] < 20
    # the training record: the first loss is the fp64 loss of the initial head on the first batch, and the loss falls
    sp = G.species_of()["train_seen"]
    tr = G.synth("train_seen")[0]
    t0 = np.array([g["label_map"][f"s{int(s)}"] for s in sp[:g["batch"]]])
    r0 = restated(tr[:g["batch"]], g["head0"]["weight"], g["head0"]["bias"], t0)
    assert abs(r0["loss"] - g["step_losses"][0]) < 1e-5
    steps = -(-len(sp) // g["batch"])
    assert len(g["step_losses"]) == steps * g["epochs"] and g["step_losses"][-1] < 0.1 * g["step_losses"][0]
    assert len(g["epoch_losses"]) == g["epochs"] == len(g["evaluation"])
    np.testing.assert_allclose(g["epoch_losses"], g["step_losses"].reshape(g["epochs"], steps).mean(axis=1), rtol=1e-12)
    # evaluate_epoch's dict from the recorded indices
    t = np.array([g["label_map"][f"s{int(s)}"] for s in g["species"]["seen_query"]])
    idx = g["idx"]["seen_query"].astype(np.int64)
    for kk in (1, 3, 5):
        assert g["final_evaluation"][f"top{kk}_accuracy"] == np.mean(np.any(idx[:, :kk] == t[:, None], axis=1))
    assert g["final_evaluation"]["top1_accuracy"] < 1.0


def test_host_helpers_and_grid_agree_with_the_golden(golden):
    from clibd_amd import method_linear as ML
    from clibd_amd import method_nn as NN

    G = _gen()
    g = golden
    loader = G.loader_of("train_seen", G.synth("train_seen")[0], g["batch"], torch.from_numpy)
    label_map, idx_to_all = ML.load_all_seen_species_name_and_create_label_map(loader)
    assert label_map == g["label_map"] and idx_to_all == g["idx_to_all_labels"]
    assert list(label_map) == sorted(label_map) and len(label_map) == 36          # sorted as strings: s0, s1, s10, ...
    batch = loader[0][6]
    t = ML.label_batch_to_species_idx(batch, label_map)
    assert t.dtype == torch.int64 and t.tolist() == [label_map[s] for s in batch["species"]]
    with pytest.raises(KeyError):
        ML.label_batch_to_species_idx({"species": ["s36"]}, label_map)
    assert sorted(ML.get_all_unique_species_from_dataloader(loader)) == sorted(label_map)
    # the grid: 1 001 points, one more than method_nn's
    grid = ML.threshold_grid()
    assert grid.shape == (1001,) and np.array_equal(grid, np.linspace(0, 1, 1001)) and NN._grid(1000, None).shape == (1000,)
    assert g["best"] in grid.tolist() and g["num_intervals"] == 1000
    # the reference's arg-max over the recorded counts
    Qs, Qu = g["cfg"]["n_seen"], g["cfg"]["n_unseen"]
    assert g["hits"].shape == (1001, 2)
    assert NN.choose_threshold(g["hits"], [Qs, Qu], grid) == g["best"]
    curve = NN.harmonic_curve(g["hits"], [Qs, Qu])
    assert len(set(curve)) >= 50 and 0 < grid.tolist().index(g["best"]) < 1000
    tb = grid.tolist().index(g["best"])
    assert g["hits"][tb, 0] / Qs >= 0.3 and g["hits"][tb, 1] / Qu >= 0.3
    assert g["out"]["seen"]["micro_acc"][1]["species"] == g["hits"][tb, 0] * 1.0 / Qs
    assert g["out"]["unseen"]["micro_acc"][1]["species"] == g["hits"][tb, 1] * 1.0 / Qu
    assert g["out"]["seen"]["best_threshold"] == g["best"] and g["out_at"]["seen"]["best_threshold"] == g["given_threshold"] != g["best"]
