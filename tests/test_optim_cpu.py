"""CPU checks of the optimizer's clipping, groups and skip (clibd_amd.optim, include/clibd_hip_optim.h): the thirteenth header and its
binding table, every host refusal of the entries, the unit's resource report, the constructor's refusals, HF Trainer's decay rule against
transformers' own helper, the norm restatements of tests/optim_reference.py, and the documents."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import optim_reference as OR  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_optim.h"
SYMBOLS = ["clibd_adam_l2_step_groups", "clibd_adamw_step_groups", "clibd_grad_norm", "clibd_grad_norm_workspace_bytes"]
KERNELS = ["grad_sumsq_kernel", "grad_norm_finish_kernel", "adam_groups_kernelILb0", "adam_groups_kernelILb1"]
TINY = dict(vocab_size=259, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, max_position_embeddings=136)


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


# ---- header, binding, build -------------------------------------------------------------------------------------------------------------
def test_optim_header_symbols_opening_comment_build_unit_and_constants():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    assert "clibd_adamw_step" in _lib.HEADERS["clibd_hip.h"] and "clibd_adam_l2_step" in _lib.HEADERS["clibd_hip_simclr.h"]   # the plain entries stay where they were
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening and "no float atomic" in opening
    assert "optim" in build.SOURCES and build.SOURCES[-1] == "rollout" and HEADER in build._deps()
    assert ctypes.sizeof(_lib.OptimGroup) == 16 and _lib.OPTIM_MAX_GROUPS == 8
    assert f"#define CLIBD_GRAD_NORM_CHUNK {OR.CHUNK}" in HEADER.read_text()


def test_optim_unit_uses_no_scratch():
    """the compiler's resource remark for every kernel of optim.hip: four kernels (the update in its two forms), no scratch"""
    from clibd_amd import build

    out = [(k["name"], k["scratch"]) for k in build.resource_usage("optim")]
    assert len(out) == len(KERNELS) and all(any(k in n for n, _ in out) for k in KERNELS), out
    assert not [(n, s) for n, s in out if s != 0], out


def test_host_validation_needs_no_gpu(lib):
    """every refusal happens before any launch: the device pointers below are never dereferenced"""
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, b, c, d, r, w = P(1 << 12), P(1 << 14), P(1 << 16), P(1 << 18), P(1 << 20), P(1 << 24)

    def refused(call, cases, prefix):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            msg = L.clibd_last_error()
            assert msg.startswith(prefix) and word in msg, (kw, msg)

    ws_of = L.clibd_grad_norm_workspace_bytes
    assert ws_of(0) == 256 and ws_of(1) == 256 and ws_of(64 * OR.CHUNK) == 256 and ws_of(64 * OR.CHUNK + 1) == 512
    assert ws_of(257 * OR.CHUNK + 3) == 258 * 4 // 256 * 256 + 256

    def norm(g=a, n=100000, gs=1.0, mx=1.0, skip=0, rec=r, ws=w, ws_bytes=256):
        return L.clibd_grad_norm(g, n, gs, mx, skip, rec, ws, ws_bytes, None)

    refused(norm, [(dict(g=None), b"null"), (dict(rec=None), b"null"), (dict(ws=None, ws_bytes=0), b"null"),
                   (dict(ws=None), b"workspace size without a workspace"), (dict(ws=P((1 << 24) + 8)), b"too small or misaligned"),
                   (dict(ws_bytes=0), b"too small or misaligned"), (dict(n=65 * OR.CHUNK), b"clibd_grad_norm_workspace_bytes"),
                   (dict(mx=-1.0), b"max_norm"), (dict(mx=float("nan")), b"max_norm"), (dict(g=P((1 << 12) + 4)), b"misaligned"),
                   (dict(rec=P((1 << 20) + 2)), b"misaligned")], b"grad_norm:")
    assert norm(n=0) == 0 and norm(n=0, mx=0.0, skip=1) == 0                       # nothing to do, nothing launched

    def table(*rows):
        return (_lib.OptimGroup * len(rows))(*[_lib.OptimGroup(*row) for row in rows])

    one = table((0, 1e-3, 1e-2))
    three = table((0, 1e-3, 1e-2), (64, 2e-3, 0.0), (192, 3e-3, 0.1))
    nine = table(*[(64 * k, 1e-3, 0.0) for k in range(9)])
    for entry, prefix in ((L.clibd_adamw_step_groups, b"adamw_step_groups:"), (L.clibd_adam_l2_step_groups, b"adam_l2_step_groups:")):
        def step(p=a, g=b, m=c, v=d, n=1024, groups=three, ng=3, step=1, rec=r, entry=entry):
            return entry(p, g, m, v, n, ctypes.cast(groups, P) if groups is not None else None, ng, 0.9, 0.999, 1e-8, step, 1.0, rec, None)

        refused(step, [(dict(p=None), b"null"), (dict(g=None), b"null"), (dict(m=None), b"null"), (dict(v=None), b"null"), (dict(groups=None), b"null"),
                       (dict(step=0), b"step must be >= 1"), (dict(step=-3), b"step must be >= 1"), (dict(ng=0), b"1..8"),
                       (dict(groups=nine, ng=9), b"1..8"), (dict(groups=table((0, 1e-3, 0.0), (192, 1e-3, 0.0), (64, 1e-3, 0.0))), b"ascending"),
                       (dict(groups=table((0, 1e-3, 0.0), (64, 1e-3, 0.0), (64, 1e-3, 0.0))), b"ascending"),
                       (dict(groups=table((0, 1e-3, 0.0), (100, 1e-3, 0.0), (192, 1e-3, 0.0))), b"multiples of 64"),
                       (dict(groups=table((64, 1e-3, 0.0)), ng=1), b"start at 0"), (dict(n=192), b"below n"),
                       (dict(p=P((1 << 12) + 4)), b"misaligned"), (dict(g=P((1 << 14) + 8)), b"misaligned"), (dict(m=P((1 << 16) + 4)), b"misaligned"),
                       (dict(v=P((1 << 18) + 4)), b"misaligned"), (dict(rec=P((1 << 20) + 1)), b"misaligned")], prefix)
        assert step(n=0) == 0 and step(n=0, groups=one, ng=1, rec=None) == 0      # n == 0 is OK


# ---- the optimizer's constructor, the decay rule -------------------------------------------------------------------------------------------
def test_constructor_refusals_on_cpu_tensors():
    """the new refusals come before the device check, so CPU tensors reach them; a well-formed request on CPU tensors still ends in the
    device refusal it always ended in"""
    from clibd_amd.optim import FusedAdam, FusedAdamW

    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(10)]
    for cls in (FusedAdamW, FusedAdam):
        for bad in (0, 0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="max_grad_norm"):
                cls(ps, max_grad_norm=bad)
        with pytest.raises(ValueError, match="nonfinite"):
            cls(ps, nonfinite="raise")
        with pytest.raises(ValueError, match="at most 8"):
            cls([{"params": [p]} for p in ps[:9]])
        with pytest.raises(ValueError, match="betas and eps"):
            cls([{"params": ps[:1]}, {"params": ps[1:2], "betas": (0.8, 0.999)}])
        with pytest.raises(ValueError, match="betas and eps"):
            cls([{"params": ps[:1]}, {"params": ps[1:2], "eps": 1e-6}])
        with pytest.raises(ValueError, match="one GPU"):
            cls([{"params": ps[:1], "lr": 1.0}, {"params": ps[1:2], "weight_decay": 0.0}], max_grad_norm=1.0, nonfinite="skip")
        with pytest.raises(ValueError, match="no trainable"):
            cls([{"params": [torch.nn.Parameter(torch.zeros(2), requires_grad=False)]}])


@pytest.mark.parametrize("tied", [True, False])
def test_decay_parameter_groups_follow_hf_trainer(tied):
    """HF Trainer's rule on its own model: transformers.trainer_pt_utils.get_parameter_names(model, [nn.LayerNorm]) minus the biases takes
    weight decay, everything else none — over named_parameters(), as Trainer.create_optimizer walks them, so a tied weight counts once."""
    from transformers import BertConfig
    from transformers import BertForMaskedLM as HFBert
    from transformers.trainer_pt_utils import get_parameter_names

    from clibd_amd import mlm
    from clibd_amd.model import BertConfigLite, BertForMaskedLM
    from clibd_amd.optim import decay_parameter_groups, decay_parameter_names

    hf = HFBert(BertConfig(tie_word_embeddings=tied, pad_token_id=None, **TINY))
    allowed = {n for n in get_parameter_names(hf, [torch.nn.LayerNorm]) if not n.endswith("bias")}
    hf_decay = {n for n, _ in hf.named_parameters() if n in allowed}
    hf_exempt = {n for n, _ in hf.named_parameters() if n not in allowed}
    model = mlm.BarcodeBERTForPreTraining(BertForMaskedLM(BertConfigLite(**TINY)), tie_word_embeddings=tied)
    decay, exempt = decay_parameter_names(model)
    assert set(decay) == hf_decay and set(exempt) == hf_exempt and len(decay) == len(set(decay)) and not set(decay) & set(exempt)
    assert ("cls.predictions.decoder.weight" in decay) == (not tied) and "bert.embeddings.word_embeddings.weight" in decay
    assert "bert.embeddings.LayerNorm.weight" in exempt and "cls.predictions.transform.LayerNorm.weight" in exempt
    groups = decay_parameter_groups(model, 0.05)
    named = dict(model.named_parameters())
    assert [g["weight_decay"] for g in groups] == [0.05, 0.0]
    assert [id(p) for p in groups[0]["params"]] == [id(named[n]) for n in decay] and [id(p) for p in groups[1]["params"]] == [id(named[n]) for n in exempt]
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(ids) == len(set(ids)) == len(list(model.parameters()))                       # every parameter once, the tied ones too
    named["bert.embeddings.position_embeddings.weight"].requires_grad_(False)               # frozen parameters are left out
    assert "bert.embeddings.position_embeddings.weight" not in decay_parameter_names(model)[0]
    only_ln = decay_parameter_groups(torch.nn.LayerNorm(8), 0.1)                            # an empty group is not returned
    assert len(only_ln) == 1 and only_ln[0]["weight_decay"] == 0.0 and len(only_ln[0]["params"]) == 2


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------
def test_norm_restatements_agree_and_follow_the_documented_order():
    for n in OR.NORM_SIZES[:-1] + [300 * OR.CHUNK + 7]:
        g = OR.gradient(n)
        for gs in (1.0, 0.25):
            ref, gate, err32 = OR.norm_gate(g, gs)
            assert ref > 0 and err32 < 1e-6 and OR.NORM_FLOOR <= gate < 3e-6, (n, gs, err32)
    assert OR.partials_fp32(OR.gradient(3 * OR.CHUNK + 5)).shape == (4,)
    ones = np.ones(2 * OR.CHUNK + 1, dtype=np.float32)                                   # exact in any order
    assert OR.partials_fp32(ones).tolist() == [OR.CHUNK, OR.CHUNK, 1.0] and float(OR.norm_fp32_kernel_order(ones, 0.5)) == np.float32(0.5 * np.sqrt(2 * OR.CHUNK + 1))
    # the order is the documented one: thread 0's first value is added before its second (a sum whose result depends on it)
    g = np.zeros(OR.CHUNK, dtype=np.float32)
    g[0], g[1], g[2] = 4096.0, 1.0, 1.0                                                  # 2^24 + 1 + 1 in fp32: 2^24 left to right, 2^24 + 2 reversed
    assert float(OR.partials_fp32(g)[0]) == 2.0 ** 24 and float(OR.partials_fp32(g[::-1].copy())[0]) == 2.0 ** 24 + 2
    assert float(OR.clip_coef(np.float32(4.0), 1.0)) == float(np.float32(1.0) / (np.float32(4.0) + np.float32(1e-6)))
    assert float(OR.clip_coef(np.float32(0.5), 1.0)) == 1.0 and float(OR.clip_coef(np.float32(0.0), None)) == 1.0
    assert np.isnan(OR.clip_coef(np.float32("nan"), 1.0)) and float(OR.clip_coef(np.float32("inf"), 1.0)) == 0.0


# ---- documents -----------------------------------------------------------------------------------------------------------------------------
def test_documents_and_docstrings_say_what_is_built_and_what_is_not():
    from clibd_amd import optim

    refused = ("norm types other than 2", "clipping by value", "per-group betas or eps", "amsgrad", "maximize", "more than 8 groups", "LAMB",
               "LARS", "gradient accumulation", "device-side step counter")
    for word in refused + ("max_grad_norm", "nonfinite", "propagate", "skip", "bias correction counts the skipped step", "GradScaler",
                           "bucket_params", "decay_parameter_groups", "no new collective", "grad_norm", "skipped_steps"):
        assert word in optim.__doc__, word
    design = (ROOT / "DESIGN.md").read_text()
    assert design.index("3.16") < design.index("3.17")
    sec = design[design.index("3.17"):]
    for word in refused + ("optim.hip", "clibd_hip_optim.h", "16 384", "fp64", "no float atomic", "skip_now", "bias correction counts the skipped step",
                           "GradScaler", "VGPR", "scratch", "Occupancy", "measured", "profiles/optim.log", "bench_optim.py", "contract"):
        assert word in sec, word
    assert "max_grad_norm" in (ROOT / "README.md").read_text() and "decay_parameter_groups" in (ROOT / "README.md").read_text()
    assert "max_grad_norm" in (ROOT / "INTEGRATION.md").read_text()
    assert (ROOT / "tools" / "bench_optim.py").exists()
