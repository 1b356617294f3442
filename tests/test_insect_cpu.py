"""CPU checks of the INSECT / BZSL workflow: the seventh header (include/clibd_hip_insect.h) and its binding table, host-side validation of
the two C entries, the unit's register report, the host helpers of clibd_amd.insect, and the fixture (tests/golden/insect_golden.pt, made
by tests/golden/make_insect_golden.py from the reference's own lines) against the row-order restatement of tests/insect_reference.py."""
import ctypes
import functools
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import insect_reference as IR  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_insect.h"
SYMBOLS = ["clibd_class_mean_f32", "clibd_class_mean_workspace_bytes", "clibd_logits_topk"]


@functools.lru_cache(maxsize=None)
def gen():
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    spec = importlib.util.spec_from_file_location("make_insect_golden", ROOT / "tests" / "golden" / "make_insect_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "insect_golden.pt", weights_only=False)


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_insect_header_symbols_opening_comment_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert "prototypes" in build.SOURCES and HEADER in build._deps()


def test_prototypes_unit_uses_no_scratch():
    """the compiler remark that test_hot_kernels_use_no_scratch reads, on this one unit: the histogram, the scan, the fill, the sort, both
    forms of the chain kernel and the top-k (whose 8 slots per lane are named registers) keep their working sets in registers"""
    from clibd_amd import build

    out = [(k["name"], k["scratch"]) for k in build.resource_usage("prototypes")]
    assert len(out) == 7 and sum("class_mean_kernel" in n for n, _ in out) == 2, out
    for kernel in ("label_hist_kernel", "class_scan_kernel", "class_fill_kernel", "class_sort_kernel", "logits_topk_kernel"):
        assert any(kernel in n for n, _ in out), kernel
    assert not [(n, s) for n, s in out if s != 0], out


def test_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, b, c, d, e, ws = P(1 << 12), P(1 << 14), P(1 << 16), P(1 << 18), P(1 << 20), P(1 << 22)
    need = L.clibd_class_mean_workspace_bytes(100, 7)
    assert need >= 4 * (8 + 7 + 100) and need % 256 == 0
    assert L.clibd_class_mean_workspace_bytes(0, 7) == 0 == L.clibd_class_mean_workspace_bytes(100, 0) == L.clibd_class_mean_workspace_bytes(100, 65537)
    assert L.clibd_class_mean_workspace_bytes(1, 65536) > 0

    def cm(x=a, ld_x=16, labels=b, N=100, C=7, D=16, mean=c, ld_mean=16, transposed=0, count=d, error=e, w=ws, nbytes=need):
        return L.clibd_class_mean_f32(x, ld_x, labels, N, C, D, mean, ld_mean, transposed, count, error, w, nbytes, None)

    for kw, word in ((dict(x=None), b"null"), (dict(labels=None), b"null"), (dict(mean=None), b"null"), (dict(count=None), b"null"),
                     (dict(error=None), b"null"), (dict(w=None), b"null"), (dict(N=0), b"non-positive"), (dict(C=0), b"non-positive"),
                     (dict(D=0, ld_mean=16), b"non-positive"), (dict(C=65537, ld_mean=16), b"at most 65536"),
                     (dict(N=1 << 20, D=1 << 11, ld_x=1 << 11, ld_mean=1 << 11), b"below 2^31"), (dict(transposed=2), b"transposed"),
                     (dict(ld_x=15), b"ld_x"), (dict(ld_mean=15), b"ld_mean"), (dict(transposed=1, ld_mean=6), b"ld_mean"),
                     (dict(x=P((1 << 12) + 2)), b"4-byte"), (dict(nbytes=need - 1), b"clibd_class_mean_workspace_bytes"),
                     (dict(w=P((1 << 22) + 8)), b"misaligned")):
        assert cm(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())

    def tk(logits=a, ld=40, B=3, C=36, k=5, val=b, idx=c):
        return L.clibd_logits_topk(logits, ld, B, C, k, val, idx, None)

    for kw, word in ((dict(logits=None), b"null"), (dict(val=None), b"null"), (dict(idx=None), b"null"), (dict(B=0), b"non-positive"),
                     (dict(C=0), b"non-positive"), (dict(C=(1 << 24) + 1, ld=(1 << 24) + 1), b"too large"), (dict(ld=35), b"ld must be"),
                     (dict(logits=P((1 << 12) + 1)), b"4-byte"), (dict(k=0), b"1..8"), (dict(k=9), b"1..8"), (dict(C=4, k=5), b"k larger")):
        assert tk(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())


# ---- the restatement against the fixture ----------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_prototypes_and_csv(golden):
    G = gen()
    p = golden["proto"]
    assert p["sizes"] == G.PROTO_SIZES and p["seed"] == G.PROTO_SEED and min(p["sizes"]) == 1 and max(p["sizes"]) >= 64
    feats, labels = G.proto_world()
    table = IR.class_embeddings(feats, labels)
    assert table.dtype == np.float32 and table.shape == p["class_embed"].shape == (G.PROTO_D, len(G.PROTO_SIZES))
    assert np.array_equal(table.view(np.uint32), p["class_embed"].view(np.uint32))
    assert IR.savetxt_text(table) == p["text"]
    changed, total = p["reversed_changes"]
    assert changed >= total / 2 and total >= 30            # `==` would see a wrong order
    # an order other than the rows' own is seen: class means over the rows sorted by their first feature differ
    order = np.argsort(feats[:, 0], kind="stable")
    assert not np.array_equal(IR.class_embeddings(feats[order], labels[order]), table)
    # empty class, bad label
    mean, count, error = IR.class_mean(feats[:5], np.array([0, 2, 2, 7, -1]), 4)
    assert count.tolist() == [1, 0, 2, 0] and error == 1 and not mean[1].any() and np.array_equal(mean[0], feats[0])


def test_golden_is_honest(golden):
    g = golden
    assert g["step_losses"][-1] < 0.1 * g["step_losses"][0] and len(g["step_losses"]) == g["epochs"] * 3
    assert (g["eval_redraw"] > 0).sum() < 0.05 * len(g["eval_redraw"])
    assert g["ref_state_dict_keys"] == ["encoder.weight", "encoder.bias", "new_linear_layer.weight", "new_linear_layer.bias"]
    assert sorted(g["species"]) == sorted(f"s{i}" for i in range(36))
    G = gen()
    img, dna = G.MLG.synth("seen_query", g["eval_redraw"])
    target = np.array([g["species"].index(f"s{int(s)}") for s in G.MLG.species_of()["seen_query"]])
    for m, feats in (("image", img), ("dna", dna)):
        logits = torch.nn.functional.linear(torch.from_numpy(feats), torch.from_numpy(g["head"][m]["weight"]), torch.from_numpy(g["head"][m]["bias"]))
        top = np.sort(logits.numpy().astype(np.float64), axis=1)[:, ::-1][:, :6]
        assert (top[:, :-1] - top[:, 1:]).min() >= g["logit_gap"] == 1e-3
        _, idx = IR.logits_topk(logits, 5)
        assert np.array_equal(idx.numpy(), g["argsort"][m].astype(np.int64))
        acc = IR.topk_accuracies(idx.numpy(), target)
        assert {k: float(v) for k, v in acc.items()} == g["evaluation"][m]


# ---- the host helpers -------------------------------------------------------------------------------------------------------------------
def test_species_helpers():
    from clibd_amd import insect as I

    loader = [(None, None, None, None, None, None, {"species": ["b", "a", "b"]}), (None, None, None, None, None, None, {"species": ("c", "a")})]
    got = I.get_unique_species_for_seen(loader)
    assert sorted(got) == ["a", "b", "c"] and got == list(set(["b", "a", "b", "c", "a"]))      # Python's set order, as the reference
    assert I.get_unique_species_for_seen(loader, sort=True) == ["a", "b", "c"]
    lst = ["x", "y", "x", "z"]                                                                  # list.index: the first position
    t = I.label_batch_to_species_idx({"species": ["z", "x", "y"]}, lst)
    assert t.dtype == torch.int64 and t.tolist() == [lst.index("z"), lst.index("x"), lst.index("y")] == [3, 0, 1]
    assert I.label_batch_to_species_idx({"species": ["z"]}, I.species_index(lst)).tolist() == [3]
    with pytest.raises(ValueError, match="is not in list"):
        I.label_batch_to_species_idx({"species": ["q"]}, lst)
    with pytest.raises(ValueError):
        lst.index("q")
    for word in ("Out of scope", "loadmat", "method_linear_on_INSECT", "fine_tune_vitb_on_insect", "convert_acc_dict_to_wandb_dict", "on separate",
                 "set order", "float32 array"):
        assert word in I.__doc__, word


def test_construct_key_dict_and_overall_acc_against_the_golden(golden):
    from clibd_amd import insect as I

    G = gen()
    ref = golden["key_dict"]
    got = I.construct_key_dict(G.key_dict_inputs())
    assert list(got) == list(ref)
    for k, v in ref.items():
        if v is None:
            assert got[k] is None, k
        elif isinstance(v, list):
            assert got[k] == v, k
        else:
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
    assert got["all_key_features"] is None and got["all_key_features_label"] is None
    # device-convention inputs: tensors are concatenated as tensors, an absent tower stays None
    ins = G.key_dict_inputs()
    tens = [{k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()} for d in ins]
    for d in tens:
        d["encoded_language_feature"] = None
    gt = I.construct_key_dict(tens)
    assert gt["encoded_language_feature"] is None and torch.equal(gt["encoded_dna_feature"], torch.from_numpy(ref["encoded_dna_feature"]))
    assert I.overall_acc(G.overall_acc_input()) == golden["overall_acc"] == (0.625 + 0.1875) / 2
    acc = G.overall_acc_input()
    per = acc["encoded_image_feature"]["encoded_image_feature"]
    acc["encoded_image_feature"]["encoded_image_feature"] = {"seen": per["seen_val"], "unseen": per["unseen_val"]}
    assert I.overall_acc(acc) == golden["overall_acc"]


def test_module_surface_without_a_gpu():
    from clibd_amd import insect as I

    for name in ("EncoderWithExtraLayer", "fine_tuning_epoch", "fine_tuning_epoch_image_and_dna", "evaluate_epoch", "class_mean_embeddings",
                 "class_embeddings", "save_bzsl_embeddings", "construct_key_dict", "eval_phase", "overall_acc", "supervised_fine_tune"):
        assert callable(getattr(I, name)), name
    enc, lin = torch.nn.Linear(4, 4), torch.nn.Linear(4, 3)
    m = I.EncoderWithExtraLayer(enc, lin)
    assert list(m.state_dict()) == ["encoder.weight", "encoder.bias", "new_linear_layer.weight", "new_linear_layer.bias"]
    assert m.encoder is enc and m.get_feature(torch.ones(1, 4)).shape == (1, 4)
    shared = I.combined_parameters(m, I.EncoderWithExtraLayer(enc, torch.nn.Linear(4, 3)))
    assert len(shared) == 6 and len({id(p) for p in shared}) == 6            # the shared encoder's two tensors are listed once
    with pytest.raises(ValueError, match="device tensor"):                    # no CPU compute path
        I.class_mean_embeddings(torch.zeros(3, 4), np.array([0, 1, 0]))
    with pytest.raises(ValueError, match="1..8"):
        I.evaluate_epoch(m, [], "cpu", ["a"], k_values=[1, 9])
