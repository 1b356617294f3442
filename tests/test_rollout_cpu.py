"""CPU checks of the attention rollout: the sixth header (include/clibd_hip_rollout.h) and its binding table, host-side validation of the
three C entries, the unit's register report, the layer-window helper, the stated divergences that raise, and the fixture
(tests/golden/rollout_golden.pt, made by tests/golden/make_rollout_golden.py from the reference's own `rollout` functions) against the
fp64 restatement of tests/rollout_reference.py."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import rollout_reference as RR  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_rollout.h"
SYMBOLS = ["clibd_attn_fused_maps", "clibd_rollout_chain", "clibd_rollout_discard", "clibd_rollout_discard_workspace_bytes"]
# The reference runs its chain in fp32 (torch.eye is fp32): its recorded mask differs from the fp64 restatement by the fp32 error of at
# most eleven [S, S] products of row-stochastic-like matrices.  The emulation's measured error is 2e-7 .. 4e-7; a misread quirk (the
# column broadcast, the index-0 rule, k, a window) moves the mask by 1e-2 and more.
REFERENCE_FP32_ERROR = 2e-6


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "rollout_golden.pt", weights_only=False)


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_rollout_header_symbols_opening_comment_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert build.SOURCES[-1] == "rollout" and HEADER in build._deps()


def test_rollout_unit_uses_no_scratch():
    """the compiler remark that test_hot_kernels_use_no_scratch reads: every kernel of rollout.hip — the six fused-map instantiations, whose
    scores and fused set are up to 128 fp32 registers per lane, the select and the chain — keeps its working set in registers"""
    from clibd_amd import build

    out = [(k["name"], k["scratch"]) for k in build.resource_usage("rollout")]
    assert len(out) == 8 and sum("attn_fused_maps_kernel" in n for n, _ in out) == 6, out
    assert any("rollout_discard_kernel" in n for n, _ in out) and any("rollout_chain_kernel" in n for n, _ in out)
    assert not [(n, s) for n, s in out if s != 0], out


def test_rollout_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, b, ws = P(1 << 12), P(1 << 14), P(1 << 20)

    def fused(qkv=a, B=2, S=197, heads=12, fusion=1, out=b, ld=200):
        return L.clibd_attn_fused_maps(qkv, B, S, heads, fusion, out, ld, None)

    for kw, word in ((dict(qkv=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"non-positive"), (dict(heads=0), b"non-positive"),
                     (dict(S=0), b"non-positive"), (dict(S=257, ld=260), b"at most 256"), (dict(fusion=3), b"fusion"), (dict(fusion=-1), b"fusion"),
                     (dict(ld=196), b"ld must be"), (dict(ld=198), b"multiple of 4"), (dict(qkv=P((1 << 12) + 8)), b"aligned"),
                     (dict(out=P((1 << 14) + 4)), b"aligned")):
        assert fused(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())

    assert L.clibd_rollout_discard_workspace_bytes(3) == 48 and L.clibd_rollout_discard_workspace_bytes(0) == 0
    assert L.clibd_rollout_discard_workspace_bytes(-1) == 0

    def disc(maps=a, B=3, S=197, ld=200, k=100, w=ws, nbytes=48):
        return L.clibd_rollout_discard(maps, B, S, ld, k, w, nbytes, None)

    for kw, word in ((dict(maps=None), b"null"), (dict(w=None), b"null"), (dict(B=0), b"non-positive"), (dict(S=0), b"non-positive"),
                     (dict(S=257, ld=260), b"at most 256"), (dict(ld=196), b"ld must be"), (dict(k=-1), b"k must be"),
                     (dict(k=197 * 197 + 1), b"k must be"), (dict(nbytes=47), b"clibd_rollout_discard_workspace_bytes"),
                     (dict(w=P((1 << 20) + 8), nbytes=1 << 10), b"misaligned")):
        assert disc(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())

    def chain(maps=a, L_=5, B=2, S=197, ld=200, out=b):
        return L.clibd_rollout_chain(maps, L_, B, S, ld, out, None)

    for kw, word in ((dict(maps=None), b"null"), (dict(out=None), b"null"), (dict(L_=0), b"non-positive"), (dict(B=0), b"non-positive"),
                     (dict(S=1), b"2..256"), (dict(S=257, ld=260), b"2..256"), (dict(ld=196), b"ld must be")):
        assert chain(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())


# ---- the helpers and the module without a GPU ---------------------------------------------------------------------------------------------
def test_layer_windows():
    from clibd_amd import rollout as R

    assert R.select_layers(12) == [1, 2, 3, 4, 5] == RR.select_layers(12)
    assert R.select_layers(12, None, R.VIT_WINDOW) == [1, 2, 3, 4, 5]
    assert R.select_layers(12, None, R.DNA_WINDOW) == list(range(1, 12)) == RR.select_layers(12, None, RR.DNA_WINDOW)
    assert R.select_layers(4, None, R.DNA_WINDOW) == [1, 2, 3]
    assert R.select_layers(8) == [1] and R.select_layers(24) == list(range(1, 18))
    for i in (0, 3, 11):
        assert R.select_layers(12, i) == [i] == R.select_layers(12, i, R.DNA_WINDOW) == RR.select_layers(12, i)
    for n, i, w in ((7, None, R.VIT_WINDOW), (1, None, R.DNA_WINDOW), (12, 12, R.VIT_WINDOW), (12, -1, R.VIT_WINDOW), (0, None, R.DNA_WINDOW)):
        assert RR.select_layers(n, i, w) == []              # where the reference would return 0/0
        with pytest.raises(ValueError, match="no layer selected"):
            R.select_layers(n, i, w)
    assert R.discard_count(197, 0.9) == int(197 * 197 * 0.9) == 34928 == RR.discard_count(197, 0.9)
    assert R.discard_count(133, 0.9) == 15920 and R.discard_count(17, 0.9) == 260 and R.discard_count(17, 0) == 0 and R.discard_count(2, 1.0) == 4
    for bad in (-0.1, 1.01):
        with pytest.raises(ValueError):
            R.discard_count(17, bad)


def test_module_imports_and_divergences_raise_without_a_gpu():
    from clibd_amd import ops
    from clibd_amd import rollout as R
    from clibd_amd.model.image_encoder import CLIBDImageEncoder, create_vit

    for name in ("fused_attention_maps", "rollout_from_maps", "attention_rollout", "VITAttentionRollout", "BarcodeBERTAttentionRollout"):
        assert callable(getattr(R, name)), name
    for word in ("independent", "ValueError", "text tower", "NotSupportedYet", "cv2", "ascending flat index", "COLUMN j"):
        assert word in R.__doc__, word
    assert R.FUSIONS == {"mean": 0, "max": 1, "min": 2} and R.MAX_IMAGES_PER_FORWARD == 64
    assert ops.rollout_ld(197) == 200 and ops.rollout_ld(133) == 136 and ops.rollout_ld(256) == 256 and ops.rollout_ld(2) == 4
    with pytest.raises(ValueError, match="Not supported"):
        R.fused_attention_maps(torch.zeros(4, 192, dtype=torch.bfloat16), 2, 2, 1, "median")
    with pytest.raises(ValueError, match="device tensor"):      # no CPU compute path
        R.fused_attention_maps(torch.zeros(4, 192, dtype=torch.bfloat16), 2, 2, 1, "max")
    with pytest.raises(ValueError):
        R.rollout_from_maps(torch.zeros(2, 1, 5, 4), 0.9)
    with pytest.raises(TypeError, match="CLIBDImageEncoder or a CLIBDDNAEncoder"):
        R.VITAttentionRollout(torch.nn.Linear(2, 2))
    enc = CLIBDImageEncoder(create_vit("vit_base_patch16_224", num_classes=0, embed_dim=128, depth=2, num_heads=2), r=4)
    with pytest.raises(ValueError, match="Not supported"):
        R.VITAttentionRollout(enc, head_fusion="median")
    ro = R.VITAttentionRollout(enc, "attn_drop", "max", 0.5)
    assert (ro.head_fusion, ro.discard_ratio) == ("max", 0.5) and R.VITAttentionRollout(enc).head_fusion == "min"
    ro.remove_hooks()
    assert list(ro.hooks) == []


def test_discard_rule_of_the_restatement():
    F = np.array([[0.5, 0.1, 0.3], [0.1, 0.2, 0.1], [0.4, 0.1, 0.6]])
    z = RR.discard_pattern(F, 3)                 # four entries equal 0.1: the first three in flat order go
    assert np.nonzero(z.reshape(-1))[0].tolist() == [1, 3, 5]
    assert np.nonzero(RR.discard_pattern(F, 5).reshape(-1))[0].tolist() == [1, 3, 4, 5, 7]
    assert not RR.discard_pattern(F, 0).any()
    full = RR.discard_pattern(F, 9)
    assert full.sum() == 8 and not full[0, 0]     # index 0 counts among the k and keeps its value
    G = F.copy()
    G[0, 0] = 0.05                                # [0, 0] the smallest: k - 1 entries are zeroed
    assert np.nonzero(RR.discard_pattern(G, 3).reshape(-1))[0].tolist() == [1, 3]
    assert RR.discard(G, 3)[0, 0] == 0.05
    assert RR.boundary(F, 3) == (0.1, 0.0) and RR.boundary(F, 4)[1] == pytest.approx(1.0)


# ---- the fixture against the restatement ------------------------------------------------------------------------------------------------
def _a_fused(golden, dtype):
    cfg = golden["A"]["cfg"]
    S, heads = cfg["S"], cfg["heads"]
    return {f: [RR.fused_maps(RR.synth_qkv([golden["A"]["seed"], l], 1, S, heads), 1, S, heads, f, dtype)[0] for l in range(cfg["layers"])]
            for f in cfg["fusions"]}


def test_fp64_restatement_reproduces_golden_a(golden):
    """pins the column-broadcast normalisation, the index-0 rule, k = int(S * S * ratio) and both windows and reshapes"""
    cfg = golden["A"]["cfg"]
    assert (cfg["S"], cfg["heads"], cfg["layers"]) == (17, 3, 12) and len(golden["A"]["masks"]) == 24
    f64, f32 = _a_fused(golden, torch.float64), _a_fused(golden, torch.float32)
    worst = 0.0
    for (kind, fusion, ratio, li), ref in golden["A"]["masks"].items():
        layers = RR.select_layers(12, li, RR.VIT_WINDOW if kind == "vit" else RR.DNA_WINDOW)
        m64 = RR.rollout64([f64[fusion][l] for l in layers], ratio)
        assert ref.shape == ((4, 4) if kind == "vit" else (16,)) and ref.dtype == np.float32 and not np.isnan(ref).any()
        err = RR.abs_err(ref.reshape(-1), m64)
        emu = RR.abs_err(RR.rollout32([f32[fusion][l] for l in layers], ratio), m64)
        worst = max(worst, err)
        print(f"A {kind} {fusion} {ratio} {li}: reference fp32 vs fp64 restatement {err:.2e}, fp32 emulation {emu:.2e}")
        assert err <= REFERENCE_FP32_ERROR and emu <= REFERENCE_FP32_ERROR
        if li == 3 and ratio == 0.9:
            assert (ref > 0).sum() >= 2           # the single-layer mask is not 0/0
    # a transposed normalisation (each row over its own sum) is NOT what the reference computes
    S = 17
    maps =[RR.discard(f64["max"][l], RR.discard_count(S, 0.9)) for l in RR.select_layers(12, None, RR.DNA_WINDOW)]
    res = np.eye(S)
    for F in maps:
        a = (F + np.eye(S)) / 2
        res = (a / a.sum(axis=-1, keepdims=True)) @ res
    other = res[0, 1:] / res[0, 1:].max()
    assert RR.abs_err(golden["A"]["masks"][("dna", "max", 0.9, None)], other) > 1e-3
    assert golden["A"]["gap_min"] >= 64 * golden["A"]["emu_err_max"]


def test_fp64_restatement_reproduces_golden_b(golden):
    for kind, S, window, shape in (("vit", 197, RR.VIT_WINDOW, (14, 14)), ("dna", 133, RR.DNA_WINDOW, (132,))):
        g = golden["B"][kind]
        assert (g["S"], g["layers"], g["ratio"]) == (S, 12, 0.9) and g["mask"].shape == shape
        maps = RR.synth_maps(g["seed"], 12, S)
        assert maps.dtype == np.float32 and abs(float(maps[0].sum(axis=-1).max()) - 1) < 1e-5
        k = RR.discard_count(S, 0.9)
        for l in range(12):
            z = np.unpackbits(g["patterns"][l])[:S * S].astype(bool).reshape(S, S)
            assert np.array_equal(z, RR.discard_pattern(maps[l], k)) and z.sum() in (k, k - 1)       # torch.topk's own index set
            flat = np.sort(maps[l].reshape(-1))
            assert flat[k - 1] < flat[k]
        layers = RR.select_layers(12, None, window)
        m64 = RR.rollout64([maps[l].astype(np.float64) for l in layers], 0.9)
        err = RR.abs_err(g["mask"].reshape(-1), m64)
        emu = RR.abs_err(RR.rollout32([maps[l] for l in layers], 0.9), m64)
        print(f"B {kind}: reference fp32 vs fp64 restatement {err:.2e}, fp32 emulation {emu:.2e}")
        assert err <= REFERENCE_FP32_ERROR and emu <= REFERENCE_FP32_ERROR
        # the vector walk is row 0 of the matrix chain
        vec = RR.chain_vector32([RR.discard(maps[l], k) for l in layers])
        assert RR.abs_err(vec, m64) <= REFERENCE_FP32_ERROR


def test_emulation_error_of_the_fused_maps():
    """the yardstick of the device's gate, on N(0, 1) q and k: a relative error of the order of 1e-6 per entry"""
    for B, S, heads in ((1, 197, 12), (2, 17, 3)):
        qkv = RR.synth_qkv([5, S], B, S, heads)
        for fusion in ("mean", "max", "min"):
            F64 = RR.fused_maps(qkv, B, S, heads, fusion)
            err = RR.rel_err(RR.fused_maps(qkv, B, S, heads, fusion, torch.float32), F64)
            print(f"fused {fusion} S={S}: fp32 emulation relative error {err:.2e}")
            assert 0 < err < 1e-5
