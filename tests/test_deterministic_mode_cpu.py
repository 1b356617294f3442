"""Deterministic training mode, host side (no GPU): the additive C ABI of the fixed-order forms, their workspace queries and host-side
validation, and the switch's interface on the model and the trainer."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW = ["clibd_layernorm_bwd_pg_workspace_bytes", "clibd_layernorm_bwd", "clibd_layernorm_param_grads_workspace_bytes",
       "clibd_layernorm_param_grads", "clibd_batch_sum_workspace_bytes", "clibd_batch_sum_f32",
       "clibd_bert_embed_bwd_workspace_bytes", "clibd_bert_embed_bwd", "clibd_colsum_workspace_bytes", "clibd_colsum_bf16",
       "clibd_gemm_tn_colsum_workspace_bytes", "clibd_gemm_bf16_tn_splitk"]


@pytest.fixture(scope="module")
def L():
    from clibd_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_library_exports_the_ordered_forms(L):
    from clibd_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clibd_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(clibd_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.HEADERS["clibd_hip.h"] and hasattr(L, name), name
    assert _lib.ABI_VERSION == 7 and L.clibd_abi_version() == 7


def test_workspace_queries(L):
    # LayerNorm PG grid: min(ceil(M / 4), 1024) blocks of [2, H] partials
    assert L.clibd_layernorm_bwd_pg_workspace_bytes(50432, 768) == 1024 * 2 * 768 * 4
    assert L.clibd_layernorm_bwd_pg_workspace_bytes(40, 512) == 10 * 2 * 512 * 4
    assert L.clibd_layernorm_param_grads_workspace_bytes(640, 768) == 10 * 2 * 768 * 4
    assert L.clibd_layernorm_param_grads_workspace_bytes(403456, 768) == 1024 * 2 * 768 * 4
    # batch sum: 8 chunks from B = 64 on, one below
    assert L.clibd_batch_sum_workspace_bytes(2048, 197 * 768) == 8 * 197 * 768 * 4
    assert L.clibd_batch_sum_workspace_bytes(32, 768) == 768 * 4
    assert L.clibd_colsum_workspace_bytes(1000, 768) == 4 * 768 * 4 and L.clibd_colsum_workspace_bytes(10 ** 6, 64) == 256 * 64 * 4
    assert L.clibd_gemm_tn_colsum_workspace_bytes(6272, 768) == 24 * 768 * 4
    # embedding: 4 x M ints of sort buffers + 256 x tiles histogram + 2 x chunks x H partials + token-type partials (256-byte aligned pieces)
    al = lambda b: (b + 255) // 256 * 256
    M, H = 40960, 768
    want = 4 * al(M * 4) + al(256 * 40 * 4) + 2 * al(320 * H * 4) + al(512 * 2 * H * 4)
    assert L.clibd_bert_embed_bwd_workspace_bytes(M, H, 30522, 2) == want
    for q in (L.clibd_layernorm_bwd_pg_workspace_bytes(0, 768), L.clibd_batch_sum_workspace_bytes(0, 8), L.clibd_colsum_workspace_bytes(8, 0),
              L.clibd_bert_embed_bwd_workspace_bytes(0, 768, 10, 1), L.clibd_gemm_tn_colsum_workspace_bytes(0, 256)):
        assert q == 0


def test_host_side_validation_rejects_missing_or_short_workspaces(L):
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is rejected before a launch
    assert L.clibd_layernorm_bwd(p, None, p, p, p, 64, 768, None, None, None, None, p, 0, 0, 1.0, None, None, p, p, None, 16, None) == -1   # a size without a workspace
    assert b"workspace" in L.clibd_last_error()
    short = L.clibd_layernorm_bwd_pg_workspace_bytes(64, 768) - 16
    assert L.clibd_layernorm_bwd(p, None, p, p, p, 64, 768, None, None, None, None, p, 0, 0, 1.0, None, None, p, p, p, short, None) == -1
    assert b"too small" in L.clibd_last_error()
    assert L.clibd_batch_sum_f32(p, 2048, 768, p, p, 16, None) == -1
    # since ABI 7 a NULL workspace with size 0 selects the atomic form (it would launch): what stays rejected is a size without a workspace
    assert L.clibd_colsum_bf16(p, 768, 1000, 768, p, None, 16, None) == -1
    assert L.clibd_bert_embed_bwd(p, None, p, 100, 768, 30522, 2, p, p, p, 64, None) == -1
    assert b"too small" in L.clibd_last_error()
    assert L.clibd_bert_embed_bwd(p, None, p, 100, 768, 30522, 3, p, p, p, 1 << 30, None) == -1   # three token types: no ordered form
    assert L.clibd_layernorm_param_grads(p, 0, 768, p, p, 64, 768, p, p, 0, 0, 1.0, None, 16, None) == -1
    assert L.clibd_gemm_bf16_tn_splitk(p, 768, p, 768, 6272, 768, 768, p, 768, 1, p, p, 1 << 30, p, 16, None) == -1
    assert b"colsum workspace" in L.clibd_last_error()


def _tiny_model():
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, BertModel, CLIBDDNAEncoder, CLIBDImageEncoder, CLIBDLanguageEncoder, SimpleCLIP, VisionTransformer

    tiny = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)
    return SimpleCLIP(CLIBDImageEncoder(VisionTransformer(embed_dim=128, depth=2, num_heads=2, num_classes=10), 4, 128),
                      CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=1027, **tiny)), 4, 128),
                      CLIBDLanguageEncoder(BertModel(BertConfigLite(vocab_size=1000, **tiny)), 4, 128))


def _stacks(m):
    return [enc.tower().stack for enc in (m.image_encoder, m.dna_encoder, m.language_encoder)]


def test_switch_interface_and_environment_default(monkeypatch):
    import inspect

    from clibd_amd import engine
    from clibd_amd.train import Trainer

    monkeypatch.delenv("CLIBD_DETERMINISTIC", raising=False)
    m = _tiny_model()
    assert m.deterministic() is False and not any(s.deterministic for s in _stacks(m))
    assert m.set_deterministic(True) is m
    assert m.deterministic() is True and all(s.deterministic for s in _stacks(m))
    assert all(enc.tower().deterministic for enc in (m.image_encoder, m.dna_encoder, m.language_encoder))
    m.set_deterministic(False)
    assert m.deterministic() is False
    # not a numerics switch: the bench line's numerics record stays what it was
    assert "deterministic" not in engine.NUMERICS_CHOICES and all("deterministic" not in v for v in m.numerics().values())
    sig = inspect.signature(Trainer.__init__)
    assert "deterministic" in sig.parameters and sig.parameters["deterministic"].default is None

    monkeypatch.setenv("CLIBD_DETERMINISTIC", "1")
    m2 = _tiny_model()
    assert m2.deterministic() is True
    monkeypatch.setenv("CLIBD_DETERMINISTIC", "0")
    assert _tiny_model().deterministic() is False


def test_training_state_records_the_switch(tmp_path, monkeypatch):
    from clibd_amd import checkpoint

    monkeypatch.delenv("CLIBD_DETERMINISTIC", raising=False)
    m = _tiny_model().set_deterministic(True)
    path = str(tmp_path / "state.pt")
    checkpoint.save_training_state(path, m)
    st = torch.load(path, map_location="cpu", weights_only=False)
    assert st["deterministic"] is True and "numerics" in st
