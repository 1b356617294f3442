"""CPU checks of the pre-extracted-feature towers (`input_type: feature`): the eighth header (include/clibd_hip_mlp.h) and its binding table,
host-side validation of the three C entries, the unit's register report, and MLPEncoder / MLPVersionCLIP / load_clip_model against what
the reference's own classes hold (tests/golden/mlp_towers_golden.pt, made by tests/golden/make_mlp_towers_golden.py): state-dict keys,
the weights torch's default initialisation draws under the fixture's seed, the freeze / disable_lora flags."""
import ctypes
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "clibd_hip_mlp.h"
SYMBOLS = ["clibd_mlp_linear_dgrad", "clibd_mlp_linear_fwd", "clibd_mlp_linear_wgrad"]
NS = types.SimpleNamespace


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "mlp_towers_golden.pt", weights_only=False)


def _args(**mc):
    return NS(model_config=NS(**mc), bioscan_bert_checkpoint=None)


def _feature(input_dim, hidden_dim, **kw):
    return NS(input_type="feature", input_dim=input_dim, hidden_dim=hidden_dim, **kw)


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_mlp_header_symbols_opening_comment_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert "mlp" in build.SOURCES and HEADER in build._deps()


def test_mlp_unit_uses_no_scratch():
    """the compiler remark of `python -m clibd_amd.build --report` on this unit: the three roles of the one kernel template keep the
    staged float4 pairs, the fragments and the accumulators in registers, and the LDS images are the 20 KiB the design states"""
    from clibd_amd import build

    rows = {k["name"]: {"ScratchSize": k["scratch"], "LDS": k["lds"]} for k in build.resource_usage("mlp")}
    assert len(rows) == 3 and all("mlp_linear_kernel" in n for n in rows), rows
    assert all(v == {"ScratchSize": 0, "LDS": 20480} for v in rows.values()), rows


def test_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, b, c, d = P(1 << 12), P(1 << 14), P(1 << 16), P(1 << 18)

    def fwd(x=a, w=b, bias=c, B=5, N=16, K=4, relu=1, out=d):
        return L.clibd_mlp_linear_fwd(x, w, bias, B, N, K, relu, out, None)

    def dgrad(dy=a, w=b, h=c, B=5, N=16, K=4, dx=d):
        return L.clibd_mlp_linear_dgrad(dy, w, h, B, N, K, dx, None)

    def wgrad(dy=a, x=b, B=5, N=16, K=4, dw=c, db=d, acc=0):
        return L.clibd_mlp_linear_wgrad(dy, x, B, N, K, dw, db, acc, None)

    shapes = ((dict(B=0), b"non-positive"), (dict(N=0), b"non-positive"), (dict(K=0), b"non-positive"), (dict(K=6), b"multiple of 4"),
              (dict(K=501), b"multiple of 4"), (dict(N=24), b"multiple of 16"), (dict(N=8), b"multiple of 16"), (dict(K=4100), b"at most 4096"),
              (dict(N=4112), b"at most 4096"), (dict(B=(1 << 21) + 1), b"2^21"))
    for fn, name, nulls, misaligned in ((fwd, b"mlp_linear_fwd", ("x", "w", "out"), ("x", "w")),
                                        (dgrad, b"mlp_linear_dgrad", ("dy", "w", "dx"), ("dy", "w")),
                                        (wgrad, b"mlp_linear_wgrad", ("dy", "x", "dw"), ("dy", "x"))):
        for kw, word in shapes + tuple((({n: None}), b"null") for n in nulls) + tuple((({n: P((1 << 12) + 4)}), b"16-byte") for n in misaligned):
            assert fn(**kw) == -1, (name, kw)
            err = L.clibd_last_error()
            assert word in err and err.startswith(name), (kw, err)


# ---- the modules against the reference's ---------------------------------------------------------------------------------------------
def test_state_dict_keys_and_initial_weights_equal_the_reference(golden):
    from clibd_amd.model import MLPEncoder, MLPVersionCLIP, SimpleCLIP, load_clip_model

    i, h, o = golden["init_dims"]
    made = {"MLPEncoder": lambda: MLPEncoder(i, h, o), "MLPVersionCLIP": lambda: MLPVersionCLIP(i, i + 16, h, o),
            "SimpleCLIP": lambda: SimpleCLIP(MLPEncoder(input_dim=i, hidden_dim=h, output_dim=o), MLPEncoder(input_dim=i, hidden_dim=h, output_dim=o), None),
            "load_clip_model": lambda: load_clip_model(_args(output_dim=o, image=_feature(i, h), dna=_feature(i, h)))}
    for name, make in made.items():
        ref = "SimpleCLIP" if name == "load_clip_model" else name
        torch.manual_seed(golden["seed"])
        sd = make().state_dict()
        assert list(sd.keys()) == golden["keys"][ref], name
        for k, v in golden["init"][ref].items():
            assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), (name, k)
    assert golden["keys"]["MLPEncoder"] == [f"encoder.{j}.{n}" for j in (0, 2, 4) for n in ("weight", "bias")]
    assert "image_encoder.encoder.0.weight" in golden["keys"]["SimpleCLIP"] and "dna_encoder.encoder.4.bias" in golden["keys"]["SimpleCLIP"]
    enc = MLPEncoder(i, h, o)
    assert isinstance(enc.encoder, torch.nn.Sequential) and [type(m).__name__ for m in enc.encoder] == ["Linear", "ReLU", "Linear", "ReLU", "Linear"]
    # the reference's constructor defaults (model/mlp.py:12, 24)
    assert tuple(MLPEncoder(8).encoder[4].weight.shape) == (512, 512)
    m = MLPVersionCLIP()
    assert tuple(m.image_feature_encoder.encoder[0].weight.shape) == (512, 512) and tuple(m.dna_feature_encoder.encoder[0].weight.shape) == (512, 768)


def test_load_clip_model_builds_the_feature_mixes():
    """feature/feature, image/feature and feature/sequence: the two branches of the factory that raised NotImplementedError before"""
    from clibd_amd.model import CLIBDDNAEncoder, CLIBDImageEncoder, MLPEncoder, load_clip_model
    from clibd_amd.towers import MLPTower

    ff = load_clip_model(_args(output_dim=48, image=_feature(2048, 64), dna=_feature(500, 32)))
    assert isinstance(ff.image_encoder, MLPEncoder) and isinstance(ff.dna_encoder, MLPEncoder) and ff.language_encoder is None
    assert tuple(ff.image_encoder.encoder[0].weight.shape) == (64, 2048) and tuple(ff.dna_encoder.encoder[4].weight.shape) == (48, 32)
    assert isinstance(ff.dna_encoder.tower(), MLPTower) and ff.dna_encoder.tower() is ff.dna_encoder.tower()
    mixed = load_clip_model(_args(output_dim=48, image=NS(input_type="image", pre_train_model="vit_small_patch16_224"), dna=_feature(500, 32)))
    assert isinstance(mixed.image_encoder, CLIBDImageEncoder) and isinstance(mixed.dna_encoder, MLPEncoder)
    fs = load_clip_model(_args(output_dim=48, image=_feature(96, 64), dna=NS(input_type="sequence")))
    assert isinstance(fs.image_encoder, MLPEncoder) and isinstance(fs.dna_encoder, CLIBDDNAEncoder)
    # the stack-wide switches pass the stack-less towers by
    for m in (ff, mixed):
        assert m.set_deterministic(True) is m and m.enable_fp8_dgrad() is m and m.set_numerics(residual_grad="fp32") is m
        assert m.enable_fp8_forward(enabled=False) is m
        assert m.numerics()["dna_encoder"] == {"forward": "fp32-grade (split bf16)"}
    assert ff.deterministic() and ff.numerics()["image_encoder"] == {"forward": "fp32-grade (split bf16)"}
    assert mixed.numerics()["image_encoder"]["forward"] == "bf16" and mixed.numerics()["image_encoder"]["residual_grad"] == "fp32"
    mixed.set_deterministic(False)
    assert not mixed.deterministic() and mixed.dna_encoder.tower().deterministic      # the feature tower has one summation order, always
    tw = ff.image_encoder.tower()
    assert tw.invalidate_weight_images() is None and not hasattr(tw, "stack")
    lin = [ff.image_encoder.encoder[j] for j in (4, 2, 0)]
    assert [[id(p) for p in g] for g in tw.grad_groups()] == [[id(l.weight), id(l.bias)] for l in lin]
    assert [id(p) for p in tw.trainable_params()] == [id(p) for l in lin for p in (l.weight, l.bias)]


@pytest.mark.parametrize("dims", [(30, 64, 64), (0, 64, 64), (64, 40, 64), (64, 64, 24), (4100, 64, 64), (64, 4112, 64), (64, 64, 8200)])
def test_unsupported_dimensions_raise_at_construction(dims):
    from clibd_amd.engine import NotSupportedYet
    from clibd_amd.model import MLPEncoder, load_clip_model

    i, h, o = dims
    with pytest.raises(NotSupportedYet, match="MLP tower"):
        MLPEncoder(i, h, o)
    with pytest.raises(NotSupportedYet):
        load_clip_model(_args(output_dim=o, image=_feature(i, h), dna=_feature(i, h)))


def test_supported_edges_construct():
    from clibd_amd.model import MLPEncoder

    for dims in ((4, 16, 16), (500, 48, 80), (2048, 4096, 16), (4096, 16, 4096)):
        MLPEncoder(*dims)


def test_freeze_and_disable_lora_flags_as_in_the_reference():
    """reference simple_clip.py:223-245: disable_lora turns every parameter on, then `freeze` turns a tower off; without either flag an
    MLPEncoder is a fresh nn.Module, all trainable"""
    from clibd_amd.model import load_clip_model
    from clibd_amd.train import _backward_order, _gradient_reachable

    rg = lambda enc: [p.requires_grad for p in enc.parameters()]
    m = load_clip_model(_args(output_dim=48, image=_feature(96, 64), dna=_feature(500, 32)))
    assert all(rg(m.image_encoder)) and all(rg(m.dna_encoder)) and m.logit_scale.requires_grad
    m = load_clip_model(_args(output_dim=48, image=_feature(96, 64), dna=_feature(500, 32, freeze=True), disable_lora=True))
    assert all(rg(m.image_encoder)) and not any(rg(m.dna_encoder))
    ordered, counts = _backward_order(m, _gradient_reachable(m, None))
    assert counts == [[2, 2, 2], [0, 0, 0]] and len(ordered) == 7 and ordered[-1] is m.logit_scale
    assert [id(p) for p in ordered[:2]] == [id(m.image_encoder.encoder[4].weight), id(m.image_encoder.encoder[4].bias)]
    m = load_clip_model(_args(output_dim=48, image=_feature(96, 64, freeze=True), dna=_feature(500, 32, freeze=False), using_open_clip=False))
    assert not any(rg(m.image_encoder)) and all(rg(m.dna_encoder))


def test_reference_shaped_state_dict_loads_and_ours_exports(golden, tmp_path):
    """a state_dict() saved from the reference's SimpleCLIP of two MLPEncoders (the trajectory's initial weights, with DDP's prefix) loads
    strictly, and what ours exports carries exactly the reference's keys"""
    from clibd_amd.checkpoint import export_reference_state_dict, load_reference_checkpoint
    from clibd_amd.model import MLPEncoder, SimpleCLIP

    i, h, o = golden["dims"]
    ref_sd = golden["trajectory"]["init"]
    torch.save({"module." + k: v for k, v in ref_sd.items()}, tmp_path / "last.pth")
    m = SimpleCLIP(MLPEncoder(i, h, o), MLPEncoder(i, h, o), None)
    res = load_reference_checkpoint(m, str(tmp_path / "last.pth"))
    assert not res.missing_keys and not res.unexpected_keys
    out = export_reference_state_dict(m)
    assert list(out.keys()) == list(ref_sd.keys())
    assert all(torch.equal(out[k], v) for k, v in ref_sd.items())
