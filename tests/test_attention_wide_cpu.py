"""CPU checks of the 128- / 192-wide attention (include/clibd_hip_attn_wide.h, csrc/attention_wide.hip): the ninth header and its binding
table, every host refusal of the two C entries (never-dereferenced pointers), the unit's register report, the routing in TransformerStack /
the towers / the checkpoint loader, the oracle against the two reference goldens (tests/golden/make_wide_head_golden.py), and the documents."""
import ctypes
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "clibd_hip_attn_wide.h"
SYMBOLS = ["clibd_attention_wide_bwd", "clibd_attention_wide_fwd"]


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_library_exports_both_symbols(lib):
    assert all(hasattr(lib, s) for s in SYMBOLS)


def test_attn_wide_header_symbols_opening_comment_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert "attention_wide" in build.SOURCES and HEADER in build._deps()


def test_host_refusals_need_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, b, c, d = P(1 << 12), P(1 << 14), P(1 << 16), P(1 << 18)

    def fwd(qkv=a, B=2, S=133, nh=2, dh=128, out=b, lse=c, thr=0):
        return L.clibd_attention_wide_fwd(qkv, B, S, nh, dh, out, lse, 1, thr, 1.0, None)

    def bwd(qkv=a, dout=b, lse=c, B=2, S=133, nh=2, dh=128, dqkv=d, thr=0):
        return L.clibd_attention_wide_bwd(qkv, dout, lse, B, S, nh, dh, dqkv, 1, thr, 1.0, None)

    common = [(dict(qkv=None), b"null"), (dict(B=0), b"non-positive"), (dict(S=0), b"non-positive"), (dict(nh=-1), b"non-positive"),
              (dict(dh=64), b"head_dim must be 128 or 192"), (dict(dh=96), b"head_dim"), (dict(dh=256), b"head_dim"),
              (dict(S=257), b"S must be <= 256"), (dict(S=193, dh=192), b"S must be <= 192"), (dict(S=257, dh=192), b"S must be <= 192"),
              (dict(B=1 << 16, nh=1 << 16), b"grid too large"), (dict(qkv=P((1 << 12) + 8)), b"alignment"),
              (dict(thr=65536), b"dropout threshold"), (dict(thr=-1), b"dropout threshold"),
              (dict(thr=6554, B=1 << 10, nh=1 << 6, S=256), b"dropout index overflow")]
    for call, name, more in ((fwd, b"attention_wide_fwd", [(dict(out=None), b"null"), (dict(out=P((1 << 14) + 8)), b"alignment"), (dict(lse=P((1 << 16) + 2)), b"alignment")]),
                             (bwd, b"attention_wide_bwd", [(dict(dout=None), b"null"), (dict(dqkv=None), b"null"), (dict(lse=None), b"lse"),
                                                           (dict(dout=P((1 << 14) + 8)), b"alignment"), (dict(dqkv=P((1 << 18) + 4)), b"alignment")])):
        for kw, word in common + more:
            assert call(**kw) == -1, (name, kw)
            msg = L.clibd_last_error()
            assert word in msg and msg.startswith(name), (name, kw, msg)
    assert b"log-sum-exp" in (bwd(lse=None), L.clibd_last_error())[1]


def test_wide_unit_uses_no_scratch():
    """the compiler remark of `python -m clibd_amd.build --report` on this unit: every instantiation (two widths, up to sixteen key tiles, with and
    without dropout, forward with four and with eight waves, backward) keeps its score rows, operand fragments and accumulators in registers"""
    from clibd_amd import build

    rows = {k["name"]: k["scratch"] for k in build.resource_usage("attention_wide")}
    fwd, bwd = [n for n in rows if "attention_wide_fwd_kernel" in n], [n for n in rows if "attention_wide_bwd_kernel" in n]
    # (8 tile counts at 128 + 6 at 192) x {dropout, none}; the forward once more with eight waves at six and more tiles (6 + 4 tile counts)
    assert len(bwd) == 28 and len(fwd) == 28 + 20 and len(rows) == 76, sorted(rows)
    assert not {n: v for n, v in rows.items() if v != 0}


# ---- routing ----------------------------------------------------------------------------------------------------------------------------
def _dna(hidden, heads, layers=1, vocab=258):
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder

    cfg = BertConfigLite(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                         max_position_embeddings=160)
    return CLIBDDNAEncoder(BertForMaskedLM(cfg), r=4, num_classes=32)


@pytest.mark.parametrize("hidden,heads,dh", [(768, 6, 128), (768, 4, 192), (256, 2, 128), (768, 12, 64)])
def test_stack_accepts_the_three_head_widths(hidden, heads, dh):
    tower = _dna(hidden, heads).tower()
    assert tower.stack.dh == dh and tower.stack.heads == heads and tower.stack.H == hidden


def test_stack_refuses_other_head_widths_and_names_the_three():
    from clibd_amd.engine import NotSupportedYet, TransformerStack

    for hidden, heads in ((768, 5), (768, 8), (768, 24), (768, 3)):
        with pytest.raises(NotSupportedYet, match=r"64, 128 and 192"):
            _dna(hidden, heads).tower()
    assert TransformerStack.HEAD_DIMS == (64, 128, 192)


def test_wide_vit_is_refused_at_construction():
    from clibd_amd.engine import NotSupportedYet
    from clibd_amd.model.image_encoder import CLIBDImageEncoder, create_vit

    enc = CLIBDImageEncoder(create_vit("vit_base_patch16_224", num_classes=0, embed_dim=256, depth=1, num_heads=2), r=4)
    with pytest.raises(NotSupportedYet, match="head_dim 64 only"):
        enc.tower()
    CLIBDImageEncoder(create_vit("vit_base_patch16_224", num_classes=0, embed_dim=128, depth=1, num_heads=2), r=4).tower()


def test_checkpoint_with_embedded_config_builds_a_wide_tower(tmp_path):
    """the newer checkpoints carry their shape in `bert_config`: six heads at hidden 768 must load and build (4-mer vocabulary of 258 from the file)"""
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder
    from clibd_amd.model.dna_encoder import load_pre_trained_bioscan_bert

    cfg = dict(vocab_size=258, hidden_size=768, num_hidden_layers=2, num_attention_heads=6, intermediate_size=1024, max_position_embeddings=160,
               output_hidden_states=True)
    src = BertForMaskedLM(BertConfigLite(**{k: v for k, v in cfg.items() if k != "output_hidden_states"}))
    sd = {"module." + k: v for k, v in src.state_dict().items()}
    path = tmp_path / "BIOSCAN-5M-BEST_k4_6_6_w1_m0_r0.pt"
    torch.save({"model": sd, "bert_config": cfg}, path)
    model = load_pre_trained_bioscan_bert(str(path), k=4)
    assert model.config.num_attention_heads == 6 and len(model.bert.encoder.layer) == 2
    assert model.bert.embeddings.word_embeddings.weight.shape == (258, 768)
    assert torch.equal(model.bert.encoder.layer[1].attention.self.key.weight, src.bert.encoder.layer[1].attention.self.key.weight)
    tower = CLIBDDNAEncoder(model, r=4, num_classes=768).tower()
    assert tower.stack.dh == 128 and tower.stack.heads == 6 and len(tower.stack.layers) == 2


# ---- the yardstick: the oracle against the reference (passes before the feature as well) -----------------------------------------------
@pytest.mark.parametrize("dh", [128, 192])
def test_oracle_reproduces_the_wide_head_goldens(dh):
    from oracle import clibd_oracle as O
    from tests.test_oracle import check_grads

    g = torch.load(ROOT / "tests" / "golden" / f"wide_head_{dh}_golden.pt", map_location="cpu", weights_only=False)
    c = g["config"]
    assert c["hidden_size"] // c["num_attention_heads"] == dh and g["ids"].shape == (3, 133) and g["vocab"] == 258
    m = O.DNAEncoder(O.BertForMaskedLM(vocab=g["vocab"], hidden=c["hidden_size"], layers=c["num_hidden_layers"], heads=c["num_attention_heads"],
                                       ff=c["intermediate_size"], max_pos=g["max_pos"]), r=4, num_classes=128)
    m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in g["state_dict"].items()}, strict=True)
    m.eval()
    assert all(float(v.float().abs().max()) > 0 for k, v in g["state_dict"].items() if ".w_b." in k)       # adapters with non-zero B
    y = m(g["ids"])
    assert (y - g["out"]).abs().max().item() < 2e-6
    assert torch.allclose(y.sum(1), torch.ones(3), atol=1e-5)
    check_grads(m, (y * g["cot"]).sum(), g["grads"])


# ---- documents ------------------------------------------------------------------------------------------------------------------------------
def test_documents_state_the_limits():
    design = (ROOT / "DESIGN.md").read_text()
    sec = design[design.index("3.13"):]
    for word in ("attention_wide.hip", "160 KiB", "192", "key mask", "rollout", "tokenizer", "NotSupportedYet", "lse", "bit for bit"):
        assert word in sec, word
    integ = (ROOT / "INTEGRATION.md").read_text()
    for word in ("pre_train_for_barcode_bert", "tokenizer", "trust_remote_code", "int64"):
        assert word in integ, word
    assert "128" in (ROOT / "README.md").read_text() and "attention_wide" in (ROOT / "README.md").read_text()
    assert "shapes built; tokenizer out of scope" in (ROOT / "SURVEY.md").read_text()
    from clibd_amd import rollout as R

    assert "64 wide" in R.__doc__
