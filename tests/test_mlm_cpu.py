"""CPU checks of the masked-k-mer pre-training: the tenth header (include/clibd_hip_mlm.h) and its binding table, every host refusal of the
four C entries, the unit's resource report, the sampler's restatement (tests/mlm_reference.py), the HF golden
(tests/golden/mlm_golden.pt, made by tests/golden/make_mlm_golden.py from transformers.BertForMaskedLM) against the oracle in fp32 mode
plus the restated vocabulary head, the tying, and the checkpoint round trip."""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import mlm_reference as MR  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_mlm.h"
SYMBOLS = ["clibd_mlm_ce_bf16", "clibd_mlm_mask", "clibd_rows_gather_bf16", "clibd_rows_scatter_bf16"]
KERNELS = ["mlm_mask_kernel", "mlm_count_valid_kernel", "rows_gather_kernel", "rows_zero_kernel", "rows_scatter_kernel", "mlm_ce_kernel",
           "mlm_loss_kernel"]


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "mlm_golden.pt", weights_only=False)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# ---- header, binding, build -------------------------------------------------------------------------------------------------------------
def test_mlm_header_symbols_opening_comment_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert build.SOURCES[-2:] == ["mlm", "rollout"] and HEADER in build._deps()


def test_mlm_unit_uses_no_scratch():
    """the compiler's resource remark for every kernel of mlm.hip: seven kernels, no scratch"""
    from clibd_amd import build

    out = [(k["name"], k["scratch"]) for k in build.resource_usage("mlm")]
    assert len(out) == len(KERNELS) and all(any(k in n for n, _ in out) for k in KERNELS), out
    assert not [(n, s) for n, s in out if s != 0], out


def test_mlm_host_validation_needs_no_gpu(lib):
    """every refusal happens before any launch: the pointers below are never dereferenced"""
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, b, c, d, e = P(1 << 12), P(1 << 14), P(1 << 16), P(1 << 18), P(1 << 20)

    def refused(call, cases, prefix):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            msg = L.clibd_last_error()
            assert msg.startswith(prefix) and word in msg, (kw, msg)

    def mask(ids=a, B=4, S=133, seed=7, n_mask=66, masked=b, rows=c, targets=d, n_valid=e):
        return L.clibd_mlm_mask(ids, B, S, seed, n_mask, 0, 2, masked, rows, targets, n_valid, None)

    refused(mask, [(dict(ids=None), b"null"), (dict(masked=None), b"null"), (dict(rows=None), b"null"), (dict(targets=None), b"null"),
                   (dict(n_valid=None), b"null"), (dict(B=0), b"non-positive"), (dict(S=1, n_mask=1), b"2..256"), (dict(S=257), b"2..256"),
                   (dict(n_mask=0), b"1..S-1"), (dict(n_mask=133), b"1..S-1"), (dict(B=1 << 23, S=256, n_mask=1), b"2^31"),
                   (dict(ids=P((1 << 12) + 4)), b"misaligned"), (dict(masked=P((1 << 14) + 4)), b"misaligned"),
                   (dict(targets=P((1 << 18) + 4)), b"misaligned"), (dict(rows=P((1 << 16) + 2)), b"misaligned"),
                   (dict(n_valid=P((1 << 20) + 2)), b"misaligned")], b"mlm_mask:")

    def gather(x=a, M=100, H=64, rows=c, R=10, out=b):
        return L.clibd_rows_gather_bf16(x, M, H, rows, R, out, None)

    def scatter(src=a, rows=c, R=10, M=100, H=64, out=b):
        return L.clibd_rows_scatter_bf16(src, rows, R, M, H, out, None)

    for call, first, prefix in ((gather, "x", b"rows_gather_bf16:"), (scatter, "src", b"rows_scatter_bf16:")):
        refused(call, [({first: None}, b"null"), (dict(out=None), b"null"), (dict(rows=None), b"null"), (dict(R=0), b"non-positive"),
                       (dict(M=0), b"non-positive"), (dict(H=0), b"non-positive"), (dict(H=60), b"multiple of 8"),
                       ({first: P((1 << 12) + 8)}, b"misaligned"), (dict(out=P((1 << 14) + 8)), b"misaligned"),
                       (dict(rows=P((1 << 16) + 2)), b"misaligned"), (dict(M=1 << 30, H=64), b"too large")], prefix)

    def ce(logits=a, ld=1032, targets=b, R=10, V=1027, n_valid=c, row_loss=d, loss=e, correct=P(1 << 22), err=P(1 << 24)):
        return L.clibd_mlm_ce_bf16(logits, ld, targets, R, V, n_valid, row_loss, loss, correct, err, None)

    refused(ce, [(dict(logits=None), b"null"), (dict(targets=None), b"null"), (dict(n_valid=None), b"null"), (dict(row_loss=None), b"null"),
                 (dict(loss=None), b"null"), (dict(correct=None), b"null"), (dict(R=0), b"non-positive"), (dict(V=0), b"non-positive"),
                 (dict(V=8193, ld=8200), b"at most 8192"), (dict(ld=1024), b"ld must be"), (dict(ld=1028), b"multiple of 8"),
                 (dict(logits=P((1 << 12) + 8)), b"misaligned"), (dict(targets=P((1 << 14) + 4)), b"misaligned"),
                 (dict(err=P((1 << 24) + 2)), b"misaligned")], b"mlm_ce_bf16:")


# ---- the sampler's restatement ------------------------------------------------------------------------------------------------------------
def _ids(B, S, V=1027, seed=0, real=None):
    g = torch.Generator().manual_seed(seed)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1)
    for b, n in (real or {}).items():
        ids[b, 1 + n:] = 2
    return ids


def test_sampler_restatement_rule():
    B, S = 4, 133
    ids = _ids(B, S, real={1: 40, 3: 0})     # sequence 1: 40 real k-mers; sequence 3: padding only
    for ratio in (0.15, 0.5, 1.0):
        n_mask = MR.n_mask_for(S, ratio)
        masked, rows, targets, n_valid = MR.sample(ids, 99, n_mask)
        assert rows.dtype == torch.int32 and targets.dtype == torch.int64 and rows.numel() == targets.numel() == B * n_mask
        r = rows.long().view(B, n_mask)
        for b in range(B):
            s = r[b] - b * S
            assert (s >= 1).all() and (s < S).all() and (s[1:] > s[:-1]).all()              # exactly n_mask distinct positions, never 0, ascending
            chosen_unk = int((ids[b, s] == 2).sum())
            real_n = int((ids[b, 1:] != 2).sum())
            assert chosen_unk == max(0, n_mask - real_n)                                    # padding goes last
        assert (masked.view(-1)[rows.long()] == 0).all()
        keep = torch.ones(B * S, dtype=torch.bool)
        keep[rows.long()] = False
        assert torch.equal(masked.view(-1)[keep], ids.view(-1)[keep])
        orig = ids.view(-1)[rows.long()]
        assert torch.equal(targets, torch.where(orig == 2, torch.full_like(orig, MR.IGNORE), orig))
        assert int(n_valid) == int((targets != MR.IGNORE).sum()) and (targets.view(B, n_mask)[3] == MR.IGNORE).all()
        again = MR.sample(ids, 99, n_mask)
        assert all(torch.equal(x, y) for x, y in zip((masked, rows, targets, n_valid), again))
        if ratio < 1.0:
            assert not torch.equal(MR.sample(ids, 100, n_mask)[1], rows)
    assert MR.n_mask_for(2, 0.5) == 1 and MR.n_mask_for(133, 0.5) == 66 and MR.n_mask_for(133, 0.15) == 19
    m, r, t, n = MR.sample(_ids(1, 2), 5, 1)
    assert r.tolist() == [1] and int(n) == 1


def test_module_helpers_and_docstring():
    from clibd_amd import mlm

    for word in ("80/10/10", "span masking", "remote-code tokenizer", "data-parallel", "fp8", "S > 256", "labels [B, S]"):
        assert word in mlm.__doc__, word
    for S, ratio in ((2, 0.5), (17, 0.15), (133, 0.5), (133, 1.0), (256, 0.15)):
        assert mlm.n_mask_for(S, ratio) == MR.n_mask_for(S, ratio)
    with pytest.raises(ValueError):
        mlm.n_mask_for(17, 0.0)
    with pytest.raises(ValueError, match="device tensor"):        # no CPU compute path
        mlm.mask_tokens(_ids(2, 17), 0.5, seed=1)


def test_ce_emulation_alone_stays_within_the_gradient_gates_share():
    """the yardstick of the device's gradient gate on the device test's own inputs: the fp32 same-formula evaluation, rounded to bf16,
    differs from bf16(fp64 gradient) in at most 1 % of the entries, each time by the adjacent value across a near tie; its loss error
    is what the loss gate multiplies by 4"""
    for R, V, ld in MR.CE_SHAPES:
        logits, targets = MR.ce_case(R, V, ld)
        assert logits.shape == (R, ld) and (logits[:, V:] == 1.0e30).all()
        l64, row64, g64, hits64 = MR.ce_reference(logits, V, targets, torch.float64)
        l32, row32, g32, hits32 = MR.ce_reference(logits, V, targets, torch.float32)
        nz = g64 != 0
        emu_rel = float(((g32.double() - g64).abs()[nz] / g64.abs()[nz]).max())
        ok, ndiff = MR.bf16_neighbours_ok(g32.to(torch.bfloat16), g64, 4 * max(emu_rel, 2.0 ** -24))
        print(f"ce R={R} V={V}: emulation loss error {abs(float(l32) - float(l64)):.3e}, worst row {float((row32.double() - row64).abs().max()):.3e}, "
              f"gradient rel error {emu_rel:.3e}, {ndiff} of {g64.numel()} entries off bf16(fp64)")
        assert ok and ndiff <= 0.01 * g64.numel() and hits32 == hits64
        assert emu_rel < 1e-5 and abs(float(l32) - float(l64)) < 1e-5
        if R > 3:
            assert hits64 >= 2 and (g64[targets == MR.IGNORE] == 0).all() and (row64[targets == MR.IGNORE] == 0).all()
            x = logits[:, :V].float()
            assert x[1].argmax() in (10, V - 3) and (x[1] == x[1].max()).sum() == 2 and (x[2] == x[2].max()).sum() == 2


# ---- the HF golden against the oracle (fp32) and the restated head ---------------------------------------------------------------------------
def _lite_shapes(cfg):
    from clibd_amd.model import BertConfigLite, BertForMaskedLM

    return {k: tuple(v.shape) for k, v in BertForMaskedLM(BertConfigLite(**cfg)).state_dict().items()}


def _golden_state(g):
    sd = MR.synth_state(g["seed"], _lite_shapes(g["config"]))
    if g["tied"]:
        sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
        sd["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"]
    assert MR.state_hash(sd) == g["weights_sha256"]          # the very weights the HF model computed with
    return sd


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("name", ["A17", "A133", "C33"])
def test_oracle_fp32_reproduces_hf_golden(golden, name, tied):
    """tolerances: tests/test_oracle.py's for its fp32 goldens (outputs 2e-6, gradients rel 2e-4 or 1e-7 absolute)"""
    g = golden[(name, tied)]
    assert (g["targets"] == MR.IGNORE).any() and int(g["n_valid"]) == int((g["targets"] != MR.IGNORE).sum())
    m2, r2, t2, n2 = MR.sample(g["ids"], 1234 + ["A17", "A133", "C33"].index(name), g["n_mask"])
    assert torch.equal(m2, g["masked"]) and torch.equal(r2, g["rows"]) and torch.equal(t2, g["targets"]) and torch.equal(n2, g["n_valid"])
    om = MR.oracle_for(g["config"], _golden_state(g), tied)
    loss, hits = MR.mlm_loss(om, g["masked"], g["rows"], g["targets"])
    print(f"{name} tied={tied}: oracle fp32 loss {float(loss.detach()):.7f}, HF {g['loss']:.7f}")
    assert abs(float(loss.detach()) - g["loss"]) < 2e-6 and hits == g["hits"]
    grads = MR.named_grads(om, loss)
    assert sorted(grads) == sorted(g["grads"])
    for k, ref in g["grads"].items():
        got = MR.sampled(k, grads[k])
        assert rel(got, ref) < 2e-4 or (got - ref).abs().max() < 1e-7, (k, rel(got, ref))
        assert abs(float(grads[k].double().norm()) - g["grad_norms"][k]) <= 2e-4 * g["grad_norms"][k] + 1e-7, k
    if tied:
        assert torch.equal(grads["cls.predictions.decoder.weight"], grads["bert.embeddings.word_embeddings.weight"])
    else:
        assert float(grads["cls.predictions.bias"].abs().max()) == 0.0          # HF: unused when untied


# ---- tying and the checkpoint ---------------------------------------------------------------------------------------------------------------
def _lite(cfg, **extra):
    from clibd_amd.model import BertConfigLite, BertForMaskedLM

    return BertForMaskedLM(BertConfigLite(**cfg, **extra))


def test_tying_shares_parameters_and_keeps_the_hf_key_set(golden):
    from clibd_amd import mlm

    cfg = golden[("A17", True)]["config"]
    keys = sorted(golden[("A17", True)]["grads"])              # the HF model's parameter names
    tied = mlm.BarcodeBERTForPreTraining(_lite(cfg))            # default: HF's tie_word_embeddings=True
    p = tied.cls.predictions
    assert tied.tie_word_embeddings and p.decoder.weight is tied.bert.embeddings.word_embeddings.weight and p.decoder.bias is p.bias
    assert sorted(tied.state_dict()) == keys
    assert len(list(tied.parameters())) == len(keys) - 2 and all(q.requires_grad for q in tied.parameters())
    assert len(tied.trainable_params()) == len(keys) - 2 and len({id(q) for q in tied.trainable_params()}) == len(keys) - 2
    untied = mlm.BarcodeBERTForPreTraining(_lite(cfg, tie_word_embeddings=False))
    q = untied.cls.predictions
    assert not untied.tie_word_embeddings and q.decoder.weight is not untied.bert.embeddings.word_embeddings.weight and q.decoder.bias is not q.bias
    assert sorted(untied.state_dict()) == keys and len(list(untied.parameters())) == len(keys)
    assert not mlm.BarcodeBERTForPreTraining(_lite(cfg), tie_word_embeddings=False).tie_word_embeddings
    from clibd_amd.model import CLIBDDNAEncoder

    with pytest.raises(ValueError, match="span the vocabulary"):
        mlm.BarcodeBERTForPreTraining(CLIBDDNAEncoder(_lite(cfg), r=4, num_classes=128, lora_layer=[]).base_dna_encoder)


@pytest.mark.parametrize("tied", [True, False])
def test_save_pretrained_round_trips_through_the_loader(golden, tied, tmp_path):
    from clibd_amd import mlm
    from clibd_amd.model.dna_encoder import load_pre_trained_bioscan_bert

    g = golden[("A17", tied)]
    model = mlm.BarcodeBERTForPreTraining(_lite(g["config"]), tie_word_embeddings=tied)
    model.load_state_dict(_golden_state(g), strict=True)
    path = tmp_path / "barcodebert.pt"
    ckpt = mlm.save_pretrained(model, path)
    assert set(ckpt) == {"model", "bert_config"} and all(not v.is_cuda for v in ckpt["model"].values())
    assert ckpt["bert_config"] == dict(g["config"], layer_norm_eps=1e-12, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                                       tie_word_embeddings=tied)
    back = load_pre_trained_bioscan_bert(str(path), k=4)
    sd, want = back.state_dict(), model.state_dict()
    assert sorted(sd) == sorted(want) == sorted(g["grads"])
    for k in want:
        assert torch.equal(sd[k], want[k]), k
    assert back.config.hidden_size == 64 and back.config.max_position_embeddings == 136 and back.config.tie_word_embeddings == tied
