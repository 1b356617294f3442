"""CPU half of the bf16 GEMM form tests: the provenance of tests/test_gemm_forms_gpu.py's bounds, its routing mirror and its judgement.

* `restate` (tests/gemm_reference.py) stays within the worst values recorded in the GPU module, on a sample of that module's inputs;
* the Python routing mirror agrees with the constants in the sources, parsed from the .hip text;
* the magnitude sum `s` is carried through the epilogue as a brute-force loop carries it;
* the per-element judgement catches and locates three corruptions of the restatement that the whole-matrix `rel_err` of
  tests/test_ops_gpu.py passes under that file's own bounds."""
import math
import sys
from dataclasses import replace
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import gemm_reference as G  # noqa: E402
import test_gemm_forms_gpu as FG  # noqa: E402


def test_restatement_stays_within_the_recorded_worst_values():
    """every 128x128 case, the split-K and K-hole cases, and a 256x256-sized sample (cut to four m-tiles: the recorded values are maxima over
    the full shapes, so a sample can only be at or below them)"""
    sample = G.cases_128() + G.cases_128_splitk() + G.cases_128_hole()[:-1]
    cut = lambda c: replace(c, M=1029, draw_M=c.M)   # the first 1029 rows of the full case's own draws
    sample += [cut(c) for kind, c in G.cases_256_kinds() if c.K == 256 and c.bias and not c.rank]
    sample += [cut(c) for _, c in G.cases_256_fold() + G.cases_256_scaled()]
    worst = G.measure_restatement(sample)
    worst["f32_acc"] = max(worst["f32_acc"], G.measure_splitk())
    seen = 0
    for cls, w in worst.items():
        assert w <= FG.WORST[cls] * (1 + 1e-4), (cls, w, FG.WORST[cls])      # (the constants are recorded to five digits)
        seen += w > 0
    assert seen == len(G.CLASSES)                      # every class is sampled
    # the small shapes' own maxima are the recorded ones for the classes they set
    for cls in ("dg_bf16", "dg_e12", "bf16_mid"):
        assert worst[cls] == pytest.approx(FG.WORST[cls], rel=1e-3), cls


def test_routing_mirror_agrees_with_the_sources():
    k = G.parse_constants()
    assert k["T"] == (G.T_M, G.T_N, G.T_K) and k["B"] == (G.BM, G.BN, G.BK)
    assert (k["min_m"], k["min_tiles"], k["ws_group"]) == (G.MIN_M_256, G.MIN_TILES_256, G.WS_GROUP)
    assert k["nk_min"] == 4 and k["splitk_nk_min"] == 8
    C = G.Case
    base = dict(out_bf16=True, bias=True)
    assert G.takes_256(C(1024, 8192, 256, **base)) and not G.takes_256(C(1023, 8192, 256, **base))                 # M >= 1024
    assert G.takes_256(C(127 * 256 + 5, 256, 256, **base)) and not G.takes_256(C(126 * 256 + 5, 256, 256, **base))   # >= 128 tiles
    assert not G.takes_256(C(1797, 4096, 128, **base)) and not G.takes_256(C(1797, 4096, 320, **base))            # nk >= 4 and even
    assert not G.takes_256(C(1797, 4096 - 16, 256, **base))                                                        # N % 256
    assert not G.takes_256(C(1797, 4096, 256, out_f32=True, split_k=2))
    assert not G.takes_256(C(1797, 4096, 256, hole=(64, 64), **base))
    assert not G.takes_256(C(1797, 4096, 256, act=G.ACT_GELU_SAVE_GRAD_E12, out_bf16=True, out_f32=True))         # an e4m7 form outside its kind: kind -1
    for kind, c in G.cases_256_kinds() + G.cases_256_fold() + G.cases_256_strided() + G.cases_256_scaled() + G.cases_256_order(256) + G.cases_256_order(304):
        assert G.takes_256(c) and G.EPI_NAMES[G.epilogue_kind(c)] == kind, c.id
    for c in G.cases_128() + G.cases_128_splitk() + G.cases_128_hole():
        assert not G.takes_256(c), c.id
    for lo, hi in G.threshold_pairs():
        assert not G.takes_256(lo) and G.takes_256(hi)
    for cus in (256, 304, 64):
        tiles = [-(-c.M // 256) * (c.N // 256) for _, c in G.cases_256_order(cus)]
        assert tiles[2] >= cus + 4 and tiles[2] >= 128                                                              # some workgroup does two tiles
    assert BASE_TILES == 128 and (G.BASE_N // 256) % G.WS_GROUP != 0 and 768 // 256 < G.WS_GROUP
    # split-K planners
    assert all(G.nt_splitk_takes(*s) for s in G.NT_SPLITK_SHAPES) and not G.nt_splitk_takes(40, 256, 256) and not G.nt_splitk_takes(40, 256, 576)
    assert all(G.tn_splitk_takes(*s) for s in G.TN_SPLITK_SHAPES) and not G.tn_splitk_takes(128, 256, 256) and not G.tn_splitk_takes(200, 256, 256)
    for nk, tiles, cus in ((8, 1, 256), (10, 1, 256), (10, 2, 304), (4, 1, 256), (6, 4, 256)):
        splits, nks = G.plan_k_slices(nk, tiles, cus)
        assert nks % 2 == 0 and nks >= 4 and nk - (splits - 1) * nks >= 4 and (splits - 1) * nks < nk
    assert G.transpose_form(50, 50, 128) == "general" and G.transpose_form(256, 257, 320) == "general"
    assert G.transpose_form(256, 256, 320) == "fast64" and G.transpose_form(128, 128, 1536) == "fast256"


BASE_TILES = -(-G.BASE_M // 256) * (G.BASE_N // 256)


def test_magnitude_sum_is_carried_like_the_value():
    """`s` against a brute-force loop at a tiny shape: rank update, bias, dropout, GELU_GRAD by aux, residual"""
    c = G.Case(5, 16, 64, act=G.ACT_GELU_GRAD, bias=True, rank=True, residual=True, out_f32=True, drop=0.25, seed=3)
    ref, s, _ = G.reference(c)["out_f32"]
    d = G.draws_for(c)
    A, W, u, v, b, aux, res = (d.get(k, "cpu").double() for k in ("A", "W", "u", "v", "bias", "aux", "res"))
    p, seed = G.drop_site(c)
    fac = G.drop_factor64(seed, c.M, c.N, p, "cpu")
    assert 0 < int((fac == 0).sum()) < fac.numel()
    for m in range(c.M):
        for n in range(c.N):
            val = sum(float(A[m, k]) * float(W[n, k]) for k in range(c.K)) + sum(float(u[m, r]) * float(v[n, r]) for r in range(8)) + float(b[n])
            mag = sum(abs(float(A[m, k]) * float(W[n, k])) for k in range(c.K)) + sum(abs(float(u[m, r]) * float(v[n, r])) for r in range(8)) + abs(float(b[n]))
            x = float(aux[m, n])
            g = 0.5 * (1.0 + math.erf(x / math.sqrt(2.0))) + x * math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
            val, mag = val * float(fac[m, n]) * g + float(res[m, n]), mag * float(fac[m, n]) * abs(g) + abs(float(res[m, n]))
            assert float(ref[m, n]) == pytest.approx(val, rel=1e-12, abs=1e-13) and float(s[m, n]) == pytest.approx(mag, rel=1e-12)
    # a dropped element without a residual is an exact zero with s = 0: only an exact zero meets it
    c0 = G.Case(5, 16, 64, out_f32=True, drop=0.5, seed=3)
    r0, s0, _ = G.reference(c0)["out_f32"]
    dead = r0 == 0
    assert dead.any() and bool((s0[dead] == 0).all())
    got = r0.clone()
    assert G.judge(got, r0, s0)[0] == 0.0
    got[dead] = 1e-30
    assert G.judge(got, r0, s0)[0] == float("inf")


def test_judgement_catches_and_locates_what_the_norm_ratio_passes():
    """Three corruptions of the restatement (not of a kernel) at the shape of test_gemm256_epilogue_kinds' smallest member: each moves the
    whole-matrix rel_err by less than that file's tightest bound for the form, and each is caught at its own place by `judge`."""
    M, N, K = 1797, 4096, 256
    ref_cache = {}

    def both(c):
        ref = G.reference(c, "cpu", ref_cache)
        return ref, {k: v[0].clone() for k, v in G.restate(c).items()}

    def check(c, name, got, ref, rows, cols, norm_bound):
        r, s, cls = ref[name]
        clean = G.restate(c)[name][0]
        assert G.judge(clean, r, s)[0] <= FG.BOUND[cls]                              # the uncorrupted restatement passes
        assert G.rel_err(got, r) < norm_bound                                        # the norm ratio of test_ops_gpu.py: passes
        e, idx = G.judge(got, r, s)
        m, n = divmod(idx, N)
        assert e > FG.BOUND[cls] and m in rows and n in cols, (e, m, n)              # per element: caught, and at the right place
        bad = G.judge_mask(got, r, s, FG.BOUND[cls])
        ms, ns = torch.nonzero(bad, as_tuple=True)
        assert int(ms.min()) >= rows[0] and int(ms.max()) <= rows[-1] and int(ns.min()) >= cols[0] and int(ns.max()) <= cols[-1]
        assert "tile" in G.locate(c, m, n)

    # (1) one lane's 8-column store strip of one row lands 8 columns to the right (EPI_BF16; test_gemm256_epilogue_kinds: rel_err < 5e-3)
    c = G.Case(M, N, K, out_bf16=True, bias=True)
    ref, got = both(c)
    clean = got["out_bf16"].clone()
    got["out_bf16"][1500, 2056:2064] = clean[1500, 2048:2056]
    got["out_bf16"][1500, 2048:2056] = clean[1500, 2056:2064]
    check(c, "out_bf16", got["out_bf16"], ref, range(1500, 1501), range(2048, 2064), 5e-3)
    # (2) one lane's 16-column group takes bias column n + 1 for column n: the four rows of a 128x128 tile that lane stores (load_bias16 is per lane)
    ref, got = both(c)
    b = G.draws_for(c).get("bias", "cpu")
    pre = G.restate(replace(c, out_bf16=False, out_f32=True))["out_f32"][0]
    rows4 = [700, 716, 732, 748]
    got["out_bf16"][rows4, 1024:1040] = G.bfr(pre[rows4, 1024:1040] + (b[1025:1041] - b[1024:1040])[None, :])
    check(c, "out_bf16", got["out_bf16"], ref, range(700, 749), range(1024, 1040), 5e-3)
    # (3) one 16-row group loses the rank-8 term (EPI_BF16 with the LoRA update; test_gemm256_epilogue_kinds: rel_err < 5e-3)
    c = G.Case(M, N, K, out_bf16=True, bias=True, rank=True, rank_scale=0.1)    # an adapter-sized update: a tenth of the main product
    ref, got = both(c)
    d = G.draws_for(c)
    u, v = d.get("u", "cpu").float(), d.get("v", "cpu").float()
    pre = G.restate(replace(c, out_bf16=False, out_f32=True))["out_f32"][0]
    got["out_bf16"][512:528] = G.bfr(pre[512:528] - u[512:528] @ v.T)
    check(c, "out_bf16", got["out_bf16"], ref, range(512, 528), range(0, N), 5e-3)
