"""CPU checks of the masked-LM labels (clibd_amd.mlm's HF-style call, include/clibd_hip_mlm_labels.h): the twelfth header and its binding
table, every host refusal of the entries, the unit's resource report, the statistics and the exclusions of the sampler's numpy
restatement (tests/mlm_labels_reference.py), the capacity rule, and the HF golden (tests/golden/mlm_labels_golden.pt, made by
tools/make_mlm_labels_golden.py from transformers.BertForMaskedLM with an attention mask and free labels) against the oracle in fp32."""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import mlm_labels_reference as LR  # noqa: E402
import mlm_reference as MR  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_mlm_labels.h"
SYMBOLS = ["clibd_mlm_compact_labels", "clibd_mlm_compact_workspace_bytes", "clibd_mlm_mask_bert"]
KERNELS = ["labels_count_kernel", "labels_offsets_kernel", "labels_compact_kernel", "mlm_mask_bert_kernel"]


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "mlm_labels_golden.pt", weights_only=False)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# ---- header, binding, build -------------------------------------------------------------------------------------------------------------
def test_mlm_labels_header_symbols_opening_comment_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert "mlm_labels" in build.SOURCES and build.SOURCES[-1] == "rollout" and HEADER in build._deps()


def test_mlm_labels_unit_uses_no_scratch():
    """the compiler's resource remark for every kernel of mlm_labels.hip: four kernels, no scratch"""
    from clibd_amd import build

    out = [(k["name"], k["scratch"]) for k in build.resource_usage("mlm_labels")]
    assert len(out) == len(KERNELS) and all(any(k in n for n, _ in out) for k in KERNELS), out
    assert not [(n, s) for n, s in out if s != 0], out


def test_host_validation_needs_no_gpu(lib):
    """every refusal happens before any launch: the device pointers below are never dereferenced"""
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, b, c, d, e, f, w = P(1 << 12), P(1 << 14), P(1 << 16), P(1 << 18), P(1 << 20), P(1 << 22), P(1 << 24)

    def refused(call, cases, prefix):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            msg = L.clibd_last_error()
            assert msg.startswith(prefix) and word in msg, (kw, msg)

    assert L.clibd_mlm_compact_workspace_bytes(0) == 0 and L.clibd_mlm_compact_workspace_bytes((1 << 24) + 1) == 0
    assert L.clibd_mlm_compact_workspace_bytes(1) == 256 and L.clibd_mlm_compact_workspace_bytes(2048 * 256) == 2048 * 4

    def compact(labels=a, M=1000, V=259, r_cap=128, rows=b, targets=c, n=d, overflow=e, err=f, ws=w, ws_bytes=256):
        return L.clibd_mlm_compact_labels(labels, M, V, r_cap, rows, targets, n, overflow, err, ws, ws_bytes, None)

    refused(compact, [(dict(labels=None), b"null"), (dict(rows=None), b"null"), (dict(targets=None), b"null"), (dict(n=None), b"null"),
                      (dict(overflow=None), b"null"), (dict(ws=None), b"null"), (dict(M=0), b"non-positive"), (dict(M=-5), b"non-positive"),
                      (dict(V=0), b"non-positive"), (dict(M=(1 << 24) + 1), b"2^24"), (dict(r_cap=0), b"multiple of 64"),
                      (dict(r_cap=32), b"multiple of 64"), (dict(r_cap=100), b"multiple of 64"), (dict(r_cap=-64), b"multiple of 64"),
                      (dict(r_cap=1088), b"rounded up"), (dict(labels=P((1 << 12) + 4)), b"misaligned"), (dict(targets=P((1 << 16) + 4)), b"misaligned"),
                      (dict(rows=P((1 << 14) + 2)), b"misaligned"), (dict(n=P((1 << 18) + 2)), b"misaligned"),
                      (dict(overflow=P((1 << 20) + 1)), b"misaligned"), (dict(err=P((1 << 22) + 2)), b"misaligned"),
                      (dict(ws=P((1 << 24) + 8)), b"misaligned"), (dict(ws_bytes=0), b"workspace too small"),
                      (dict(M=257 * 256, ws_bytes=1024), b"workspace too small")], b"mlm_compact_labels:")

    sp = (ctypes.c_int64 * 3)(0, 1, 2)
    spp = ctypes.cast(sp, P)

    def bert(ids=a, am=b, B=4, S=133, V=259, p=0.15, pm=0.8, pr=0.1, special=spp, ns=3, masked=c, labels=d):
        return L.clibd_mlm_mask_bert(ids, am, B, S, V, 7, p, pm, pr, 0, special, ns, masked, labels, None)

    refused(bert, [(dict(ids=None), b"null"), (dict(masked=None), b"null"), (dict(labels=None), b"null"), (dict(special=None), b"null"),
                   (dict(B=0), b"non-positive"), (dict(S=0), b"non-positive"), (dict(B=1 << 23, S=256), b"2^31"), (dict(ns=9), b"0..8"),
                   (dict(ns=-1), b"0..8"), (dict(V=3), b"exceed"), (dict(p=1.5), b"probabilities"), (dict(p=-0.1), b"probabilities"),
                   (dict(p=float("nan")), b"probabilities"), (dict(pm=0.95, pr=0.1), b"probabilities"), (dict(pr=-0.5), b"probabilities"),
                   (dict(ids=P((1 << 12) + 4)), b"misaligned"), (dict(masked=P((1 << 16) + 4)), b"misaligned"),
                   (dict(labels=P((1 << 18) + 4)), b"misaligned"), (dict(am=P((1 << 14) + 2)), b"misaligned")], b"mlm_mask_bert:")


# ---- the sampler's restatement ------------------------------------------------------------------------------------------------------------
def _sigma(p, n):
    return math.sqrt(p * (1 - p) / n)


@pytest.mark.parametrize("seed", [20251, 0x9E3779B9, 7])
def test_restatement_statistics(seed):
    """2^16 eligible tokens at p = 0.15: the chosen fraction within 4 binomial standard deviations of p; among the chosen, <MASK>, a
    changed id and an unchanged id within 4 standard deviations of 0.8, 0.1 (1 - 1 / (V - 3)) and 0.1 (1 + 1 / (V - 3)): a replacement
    draw is uniform over the V - 3 plain ids and equals the original with probability 1 / (V - 3), which counts as unchanged."""
    V, B, S = 259, 512, 129                                   # 128 eligible positions per sequence: 2^16 in all
    g = torch.Generator().manual_seed(1)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1).numpy()
    masked, labels = LR.sample_bert(ids, None, V, seed)
    chosen = labels != LR.IGNORE
    n_el = B * (S - 1)
    assert n_el == 1 << 16 and not chosen[:, 0].any()
    frac = chosen.sum() / n_el
    assert abs(frac - 0.15) <= 4 * _sigma(0.15, n_el), frac
    n = int(chosen.sum())
    assert (labels[chosen] == ids[chosen]).all() and (masked[~chosen] == ids[~chosen]).all()
    is_mask = masked[chosen] == 0
    same = masked[chosen] == ids[chosen]
    other = ~is_mask & ~same
    assert (masked[chosen][other] >= 3).all() and (masked[chosen][other] < V).all()
    q = 1.0 / (V - 3)
    for got, want in ((is_mask.sum() / n, 0.8), (other.sum() / n, 0.1 * (1 - q)), (same.sum() / n, 0.1 * (1 + q))):
        assert abs(got - want) <= 4 * _sigma(want, n), (got, want)


def test_restatement_exclusions_and_plain_masking():
    V, B, S = 259, 64, 133
    g = torch.Generator().manual_seed(2)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(0, V, (B, S - 1), generator=g)], dim=1).numpy()   # specials inside
    mask = (torch.rand(B, S, generator=g) > 0.3).long().numpy()
    for p in (0.15, 1.0):
        masked, labels = LR.sample_bert(ids, mask, V, 99, p=p)
        chosen = labels != LR.IGNORE
        assert not chosen[:, 0].any() and not chosen[mask == 0].any() and not chosen[ids < 3].any()
        if p == 1.0:
            assert (chosen == ((mask != 0) & (ids >= 3) & (np.arange(S)[None, :] > 0))).all()       # every eligible position
        assert (masked[~chosen] == ids[~chosen]).all()
        again = LR.sample_bert(ids, mask, V, 99, p=p)
        assert (again[0] == masked).all() and (again[1] == labels).all()
        other = LR.sample_bert(ids, mask, V, 100, p=p)
        assert not (other[0] == masked).all() and (p == 1.0 or not (other[1] == labels).all())     # at p = 1 every seed labels the same set
    masked, labels = LR.sample_bert(ids, mask, V, 5, p=0.5, replace=(1.0, 0.0, 0.0))
    chosen = labels != LR.IGNORE
    assert chosen.sum() > 1000 and (masked[chosen] == 0).all()
    masked, labels = LR.sample_bert(ids, mask, V, 5, p=0.5, replace=(0.0, 0.0, 1.0))
    assert (masked == ids).all() and (labels != LR.IGNORE).sum() == chosen.sum()
    none, lab0 = LR.sample_bert(ids, mask, V, 5, p=0.0)
    assert (none == ids).all() and (lab0 == LR.IGNORE).all()
    # the same bits whatever the batch is cut into: position i depends on (seed, i) only
    m1, l1 = LR.sample_bert(ids.reshape(1, -1)[:, :S * 2].reshape(2, S), None, V, 11)
    m2, l2 = LR.sample_bert(ids[:1], None, V, 11)
    assert (m1[0] == m2[0]).all() and (l1[0] == l2[0]).all()


def test_capacity_rule_and_compaction_restatement():
    from clibd_amd import ops

    for M, p in ((2, 0.15), (51, 0.15), (665, 0.15), (256 * 133, 0.15), (2048 * 256, 0.15), (1000, 0.0), (1000, 1.0), (1000, 0.5), (64, 0.9)):
        want = math.ceil(M * min(1.0, p + 6.0 * math.sqrt(p * (1 - p) / M)))
        want = min((M + 63) // 64 * 64, max(64, (want + 63) // 64 * 64))
        assert ops.mlm_label_capacity(M, p) == LR.capacity(M, p) == want and want % 64 == 0
        assert ops.mlm_label_capacity(M) == LR.capacity(M) == (M + 63) // 64 * 64
    assert ops.mlm_label_capacity(256 * 133, 0.15) == 5504          # 5107.2 expected, sigma 65.9: 5502.5 -> 5503 -> 5504
    labels = np.full(300, LR.IGNORE, dtype=np.int64)
    labels[[0, 7, 299]] = [5, 6, 7]
    rows, targets, n, over = LR.compact(labels, 64)
    assert rows[:3].tolist() == [0, 7, 299] and (rows[3:] == -1).all() and targets[:3].tolist() == [5, 6, 7] and (targets[3:] == -100).all()
    assert n == 3 and not over and LR.compact(np.zeros(300, dtype=np.int64), 64)[2:] == (300, True)


def test_module_docstring_and_refusals():
    from clibd_amd import mlm

    for word in ("80/10/10", "labels [B, S]", "attention_mask", "label_capacity", "label_overflow", "0x9E3779B9", "NotSupportedYet"):
        assert word in mlm.__doc__, word
    design = (ROOT / "DESIGN.md").read_text()
    sec = design[design.index("3.16"):]
    for word in ("mlm_labels.hip", "80/10/10", "six binomial standard deviations", "label_overflow", "key mask", "span", "S > 256", "fp8",
                 "data-parallel", "remote-code tokenizer", "measured"):
        assert word in sec, word
    ids = torch.zeros(2, 17, dtype=torch.long)
    with pytest.raises(ValueError, match="device tensor"):        # no CPU compute path
        mlm.mask_tokens_bert(ids, vocab_size=259, seed=1)
    with pytest.raises(ValueError, match="vocab_size"):
        mlm.mask_tokens_bert(ids, seed=1)
    ids[0, 5:] = 2
    ids[1, 3] = 2
    ids[1, 4:] = 7
    am = mlm.barcode_attention_mask(ids)
    assert am.dtype == torch.int32 and am[0].tolist() == [1] * 5 + [0] * 12 and am[1].tolist() == [1] * 17      # an inner <UNK> stays live
    ids[1] = 2
    assert mlm.barcode_attention_mask(ids)[1].tolist() == [1] + [0] * 16                                        # position 0 is always live


# ---- the HF golden against the oracle (fp32) ---------------------------------------------------------------------------------------------------
def _golden_state(g):
    from clibd_amd.model import BertConfigLite, BertForMaskedLM

    shapes = {k: tuple(v.shape) for k, v in BertForMaskedLM(BertConfigLite(**g["config"])).state_dict().items()}
    sd = MR.synth_state(g["seed"], shapes)
    if g["tied"]:
        sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
        sd["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"]
    assert MR.state_hash(sd) == g["weights_sha256"]          # the very weights the HF model computed with
    return sd


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("name", [c[0] for c in LR.CASES])
def test_oracle_fp32_reproduces_hf_golden(golden, name, tied):
    """tolerances: tests/test_mlm_cpu.py's for its own HF golden (loss 2e-6, gradients rel 2e-4 or 1e-7 absolute)"""
    g = golden[(name, tied)]
    ids, mask, labels = LR.case_inputs(name)
    assert torch.equal(ids, g["input_ids"]) and torch.equal(mask, g["attention_mask"]) and torch.equal(labels, g["labels"])
    per_seq = (labels != LR.IGNORE).sum(dim=1).tolist()
    S = g["S"]
    assert per_seq[1] == 1 and per_seq[2] == 0 and min(per_seq[0], per_seq[3]) >= 2 and sum(per_seq) == g["n_labelled"]
    assert mask[0].all() and mask[1].tolist() == [1, 1] + [0] * (S - 2) and int(mask[2].sum()) == S // 2 and int(mask[3].sum()) == S - 3
    assert labels[3, 0] != LR.IGNORE and labels[3, S // 3 + 1] != LR.IGNORE and mask[3, S // 3 + 1] == 0
    om = MR.oracle_for(g["config"], _golden_state(g), tied)
    loss, hits = LR.labels_loss(om, ids, mask, labels)
    print(f"{name} tied={tied}: oracle fp32 loss {float(loss.detach()):.7f}, HF {g['loss']:.7f}")
    assert abs(float(loss.detach()) - g["loss"]) < 2e-6 and hits == g["hits"]
    grads = MR.named_grads(om, loss)
    assert sorted(grads) == sorted(g["grads"])
    for k, ref in g["grads"].items():
        got = MR.sampled(k, grads[k])
        assert rel(got, ref) < 2e-4 or (got - ref).abs().max() < 1e-7, (k, rel(got, ref))
        assert abs(float(grads[k].double().norm()) - g["grad_norms"][k]) <= 2e-4 * g["grad_norms"][k] + 1e-7, k
    # the mask matters: without it the loss moves
    l_nomask, _ = LR.labels_loss(om, ids, None, labels)
    assert abs(float(l_nomask.detach()) - g["loss"]) > 1e-4
