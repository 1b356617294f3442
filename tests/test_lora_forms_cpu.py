"""CPU half of the LoRA adapter form tests: the provenance of tests/test_lora_forms_gpu.py's bounds, its routing mirror and its judgement.

* the restatement (tests/lora_reference.py) stays within the worst values recorded in the GPU module on a sample of that module's inputs, sets
  the ones the sample contains, and meets every integer case exactly;
* the routing mirror's constants agree with the text of lora.hip, and ops._lora_workspace with the mirror's bytes under a made-up CU count;
* the per-element judgement catches and places three corruptions of a correct result that the whole-matrix `rel_err` gates of
  tests/test_ops_gpu.py (2e-5 on the gradients, 4e-3 on dt) pass."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import lora_reference as L  # noqa: E402
import test_lora_forms_gpu as FG  # noqa: E402


def test_restatement_stays_within_the_recorded_worst_values():
    """the cases whose operands are drawn on the host (M H <= 2^22: the same bits the GPU module launches): every VALU case, the chain tails, the
    small MFMA and two-call cases.  The fused pair's classes need M >= 131072 and are re-derived by `python tests/test_lora_forms_gpu.py --fused` only."""
    small = lambda cs: [c for c in cs if c.M * c.H <= (1 << 22)]
    sample = []
    for mode in L.MODES:
        for H in L.VALU_H:
            sample += L.cases_valu(H, mode)
        sample += small(L.cases_valu_routes(mode)) + L.cases_reduce(mode)
        for H in (128, 384, 512, 1024):
            sample += small(L.cases_mfma(H, mode, 256) + L.cases_mfma_atomic(H, mode, 256))
    sample += small(L.cases_backward_two_call(256))
    assert {L.route(c.entry, c.M, c.H, c.workspace, 256)["form"] for c in sample} == {"valu", "mfma"}
    worst = L.measure_restatement(sample, 256)        # (asserts the integer cases bit-equal to fp64)
    worst["t"] = L.measure_down_proj()
    for cls in L.CLASSES:
        assert worst[cls] <= FG.WORST[cls] * (1 + 1e-4), (cls, worst[cls], FG.WORST[cls])      # (the constants are recorded to five digits)
        assert FG.BOUND[cls] == 3.0 * FG.WORST[cls] and FG.WORST[cls] > 0
    assert all(worst[cls] > 0 for cls in L.CLASSES if cls != "dt_fused")
    for cls in ("t", "g_valu", "g_mfma_partials"):      # set by small shapes
        assert worst[cls] == pytest.approx(FG.WORST[cls], rel=1e-3), cls


def test_routing_mirror_agrees_with_the_sources():
    k = L.parse_constants()
    assert (k["lw_rows"], k["lwm_rows"], k["mfma_min_m"], k["fused_min_m"]) == (L.LW_ROWS, L.LWM_ROWS, L.MFMA_MIN_M, L.FUSED_MIN_M)
    assert k["tiles"] == L.TILES_SET and k["nch"] == L.NCH_SET and set(L.NCH_SET) <= set(k["tiles_fused"])      # (2H / 256 == H / 128)
    assert all(k[f] for f in ("want_wgrad", "want_fused_a", "groups_fused_b", "ws_copies", "ws_zero", "valu_blocks", "valu_lds", "lcm", "six_steps"))
    assert k["ring"] == 4 and k["down_cap"] == L.DOWN_PROJ_MAX_BLOCKS and k["h_max"] == L.H_MAX
    r = L.route
    for cus in (256, 304, 64):
        G = L.wgrad_groups(cus)
        assert G == (2 * cus + 5) // 6
        # wgrad: whole slabs with a workspace at any M, without one from 8192; every H / 128 in 1 .. 8; H % 128 == 64 and ragged M are VALU
        for H in range(128, 1025, 128):
            assert r("wgrad", 32, H, True, cus)["form"] == "mfma" and r("wgrad", 32, H, False, cus)["form"] == "valu"
            assert r("wgrad", 8192, H, False, cus)["form"] == "mfma" and r("wgrad", 8160, H, False, cus)["form"] == "valu"
            assert r("wgrad", 8192 + 7, H, True, cus)["form"] == "valu"
        for H in range(64, 1025, 128):
            assert r("wgrad", 8192, H, True, cus)["form"] == "valu" and L.workspace_bytes(8192, H, cus) == 0
        a = r("wgrad", 32 * (12 * G + 5), 768, True, cus)
        assert a["grid"] == ((G, 6),) and a["slabs_per_wg"] == ((12, 13),) and (a["g_b"], a["g_a"]) == (G, G) and a["used_bytes"] == G * 16 * 768 * 4 <= a["ws_bytes"]
        # backward: the fused pair from 131072 whole-slab rows at H = 512, 768, 1024 only
        for H, nch, lcm in ((512, 4, 4), (768, 6, 12), (1024, 8, 8)):
            f = r("backward", 131072, H, True, cus)
            assert (f["form"], f["nch"], f["lcm"], f["tiles"]) == ("fused", nch, lcm, H // 128)
            assert f["grid"] == ((min(cus, 4096),), (min(cus, 4096), 2)) and f["used_bytes"] == f["ws_bytes"]
            assert r("backward", 131072 - 32, H, True, cus)["form"] == "mfma" and r("backward", 131072 + 1, H, True, cus)["form"] == "valu"
        assert r("backward", 131072, 256, True, cus)["form"] == "mfma" and r("backward", 131072, 640, True, cus)["form"] == "mfma"
    assert r("backward", 131072, 768, True, 256)["slabs_per_wg"] == ((16, 16), (16, 16)) and r("backward", 131104, 768, True, 256)["slabs_per_wg"] == ((16, 17), (16, 17))
    # every case list lands where the GPU module says it does
    for cus in (256, 304):
        for mode in L.MODES:
            for H in L.VALU_H:
                assert all(r(c.entry, c.M, c.H, c.workspace, cus)["form"] == "valu" for c in L.cases_valu(H, mode))
            assert all(r(c.entry, c.M, c.H, c.workspace, cus)["form"] == "valu" for c in L.cases_valu_routes(mode))
            for H in L.MFMA_H:
                assert all(r(c.entry, c.M, c.H, c.workspace, cus)["form"] == "mfma" for c in L.cases_mfma(H, mode, cus) + L.cases_mfma_atomic(H, mode, cus))
            assert [r(c.entry, c.M, c.H, True, cus)["g_b"] for c in L.cases_reduce(mode)] == list(L.REDUCE_SLABS)
        for H in L.FUSED_H:
            assert all(r(c.entry, c.M, c.H, c.workspace, cus)["form"] == "fused" for c in L.cases_fused(H))
    assert L.valu_lds_bytes(1024) == 66176 and L.down_proj_blocks(8192) == 2048 == L.down_proj_blocks(8199) and L.down_proj_blocks(8191) == 2048 and L.down_proj_blocks(5) == 2


def test_ops_workspace_agrees_with_the_mirror(monkeypatch):
    """ops._lora_workspace under a library that answers clibd_lora_workspace_bytes with the mirror's figure for a made-up CU count: the buffer it
    allocates holds what every route writes"""
    from clibd_amd import _lib, ops

    cus = 48

    class Fake:
        @staticmethod
        def clibd_lora_workspace_bytes(M, H):
            return L.workspace_bytes(M, H, cus)

    monkeypatch.setattr(_lib, "load", lambda: Fake)
    for M, H in ((32, 128), (512, 384), (8192, 768), (32 * 49, 1024), (131072, 512)):
        ws, nb = ops._lora_workspace(M, H, "cpu", None)
        assert nb == L.workspace_bytes(M, H, cus) == min(cus, M // 32) * 16 * H * 4 and ws.numel() == nb
        for entry in ("wgrad", "backward"):
            assert L.route(entry, M, H, True, cus)["used_bytes"] <= nb
        assert ops._lora_workspace(M, H, "cpu", False) == (None, 0)
        with pytest.raises(ValueError):
            ops._lora_workspace(M, H, "cpu", torch.empty((nb - 1,), dtype=torch.uint8))
    for M, H in ((700, 128), (512, 320), (33, 1024)):
        assert ops._lora_workspace(M, H, "cpu", None) == (None, 0)


def test_judgement_catches_and_places_what_the_norm_ratio_passes():
    """Three corruptions of the restatement (not of a kernel), each under test_ops_gpu.py's own gate for the output and each caught at its place"""
    # (1) one output column off by 0.1 %: column n of dq against the four ranks, dB_q[n, 0:4] (the MFMA form without a workspace, M = 8192, H = 768)
    c = L.Case("wgrad", 8192, 768, False, "real", seed=4)
    r = L.route(c.entry, c.M, c.H, c.workspace, 256)
    dqkv, x, t, dt, init, _ = L.operands_for(c)
    refs = L.grads_reference(dqkv, x, t, dt, init)
    got = L.grads_restate(dqkv, x, t, dt, init, r["form"], r["grid"][0][0], r["grid"][0][0], False)
    ref, s = refs["dB_q"]
    cls = L.grad_class(r, False)
    assert L.judge(got["dB_q"], ref, s)[0] <= FG.BOUND[cls]
    n = int((ref - init[2].double()).norm(dim=1).argmin())
    bad = got["dB_q"].clone()
    bad[n] = init[2][n] + (bad[n] - init[2][n]) * 1.001
    assert L.rel_err(bad - init[2], ref - init[2].double()) < 2e-5                      # test_lora_wgrad_mfma_form's gate: passes
    e, idx = L.judge(bad, ref, s)
    assert e > FG.BOUND[cls] and idx // 4 == n
    assert f"n = {n}," in L.locate_mfma("dB_q", c.H, idx) and f"half = {n // 384}, 64-column tile {n % 384 // 64} " in L.locate_mfma("dB_q", c.H, idx)
    where = torch.nonzero(L.judge_mask(bad, ref, s, FG.BOUND[cls]))
    assert set(where[:, 0].tolist()) == {n}
    # (2) one 4-row lane strip of one tile taken from the neighbouring tile: rows 4g .. 4g + 3 of one dt column in one 32-row slab hold the next slab's
    c = L.Case("backward", 131072, 128, False, "real", seed=12)
    dqkv, x, t, _, init, w_dt = L.operands_for(c)
    ref, s = L.dt_reference(dqkv, w_dt)
    clean = L.dt_restate(dqkv, w_dt)
    assert L.judge(clean[:, :8], ref[:, :8], s[:, :8])[0] <= FG.BOUND["dt_gemm"]
    bad = clean.clone()
    m0, col = 32 * 1000 + 4 * 2, 5
    bad[m0:m0 + 4, col] = clean[m0 + 32:m0 + 36, col]
    assert L.rel_err(bad[:, :8], ref[:, :8]) < 4e-3                                     # test_lora_backward_one_pass_over_dq_dv's gate: passes
    e, idx = L.judge(bad[:, :8], ref[:, :8], s[:, :8])
    assert e > FG.BOUND["dt_gemm"] and idx // 8 in range(m0, m0 + 4) and idx % 8 == col
    assert "32-row slab 1000, row" in L.locate_rows("dt", idx // 8, idx % 8)
    where = torch.nonzero(L.judge_mask(bad[:, :8], ref[:, :8], s[:, :8], FG.BOUND["dt_gemm"]))
    assert set(where[:, 0].tolist()) <= set(range(m0, m0 + 4)) and set(where[:, 1].tolist()) == {col}
    # (3) one dt row rounded twice: the q and v products' 64-column partial sums rounded to bf16 before they are added and rounded again (the row where
    # that moves an element most)
    H = c.H
    parts = torch.zeros((c.M, 16))
    for j in range(0, H, 64):
        parts[:, :8] += L.bfr(dqkv[:, j:j + 64].float() @ w_dt[:8, j:j + 64].float().T + dqkv[:, 2 * H + j:2 * H + j + 64].float() @ w_dt[:8, 2 * H + j:2 * H + j + 64].float().T)
    twice = L.bfr(parts)
    row = int(((twice.double() - ref).abs() / torch.maximum(ref.abs(), s * 2.0 ** -10).clamp(min=1e-300))[:, :8].max(dim=1).values.argmax())
    bad = clean.clone()
    bad[row] = twice[row]
    assert L.rel_err(bad[:, :8], ref[:, :8]) < 4e-3
    e, idx = L.judge(bad[:, :8], ref[:, :8], s[:, :8])
    assert e > FG.BOUND["dt_gemm"] and idx // 8 == row
    assert f"m = {row}," in L.locate_rows("dt", idx // 8, idx % 8)
