"""CPU checks of the seen/unseen threshold method: the golden's features, the host finaliser (integer counts -> harmonic curve -> chosen
threshold) against the reference's recorded choice (tests/golden/method_nn_golden.pt, tests/golden/make_method_nn_golden.py),
harmonic_mean's edge cases and the host-side validation of the two C entry points (no GPU needed)."""
import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "method_nn_golden.pt"


def _gen():
    spec = importlib.util.spec_from_file_location("make_method_nn_golden", ROOT / "tests" / "golden" / "make_method_nn_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def test_golden_is_what_the_generator_describes(golden):
    gen = _gen()
    for name in ("small", "large"):
        g = golden[name]
        assert g["cfg"] == gen.SETS[name]
        for s in gen.SPLITS:
            assert gen.checksum(gen.synth(g["cfg"], s, g["redraw"].get(s))) == g["checksum"][s], (name, s)
        for s, sp in gen.species_of(g["cfg"]).items():
            assert np.array_equal(sp, g["species"][s])
    assert golden["large"]["cfg"]["n_seen_keys"] >= 4096


def test_finaliser_reproduces_reference_threshold(golden):
    from clibd_amd.method_nn import choose_threshold, harmonic_curve

    plateaus = []
    for name in ("small", "large"):
        g = golden[name]
        sizes = [g["cfg"]["n_seen"], g["cfg"]["n_unseen"]]
        for n in (1000, 1001):
            grid = np.linspace(0, 1, n)
            best = choose_threshold(g["hits"][n], sizes, grid)
            assert best == g["best"][n], (name, n)
            curve = harmonic_curve(g["hits"][n], sizes)
            t = int(np.nonzero(grid == best)[0][0])
            assert 0 < t < n - 1 and curve[t] == max(curve) and curve.index(max(curve)) == t      # the FIRST maximum, an interior one
            assert len(set(curve)) >= 50
            plateaus.append(sum(c == max(curve) for c in curve))
            assert plateaus[-1] == g["plateau"][n]
        # the accuracy the reference reported at its threshold is the count the sweep recorded there
        t = int(np.nonzero(np.linspace(0, 1, 1000) == g["best"][1000])[0][0])
        assert g["out"]["seen"]["micro_acc"][1]["species"] == int(g["hits"][1000][t, 0]) * 1.0 / sizes[0]
        assert g["out"]["unseen"]["micro_acc"][1]["species"] == int(g["hits"][1000][t, 1]) * 1.0 / sizes[1]
    assert max(plateaus) >= 2                      # the first-maximum rule is exercised


def test_finaliser_edge_cases():
    from clibd_amd.method_nn import choose_threshold

    grid = np.linspace(0, 1, 5)
    assert choose_threshold(np.zeros((5, 2), np.int32), [3, 4], grid) == grid[0]                  # an all-zero curve: the first threshold
    assert choose_threshold(np.array([[1, 0], [0, 2], [0, 0], [3, 0], [0, 0]]), [3, 4], grid) == grid[0]
    assert choose_threshold(np.array([[1, 1], [2, 2], [2, 2], [1, 3], [0, 4]]), [4, 4], grid) == grid[1]        # a plateau keeps its first threshold
    assert choose_threshold(np.array([[1], [2], [3], [3], [0]]), [4], grid) == grid[2]            # one split


def test_harmonic_mean_edge_cases():
    from clibd_amd.method_nn import harmonic_mean

    assert harmonic_mean([0.5, 0, 0.25]) == 0 and harmonic_mean([0, 0.7]) == 0 and harmonic_mean([0.3, 0.0]) == 0
    assert harmonic_mean([0.25]) == 0.25
    assert harmonic_mean([0.7]) == 1 / (0 + 1 / 0.7)
    assert harmonic_mean([0.5, 0.25]) == 2 / (1 / 0.5 + 1 / 0.25)
    assert harmonic_mean([0.885, 0.82, 0.1]) == 3 / (((0 + 1 / 0.885) + 1 / 0.82) + 1 / 0.1)      # summed left to right


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _arr(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


P = ctypes.c_void_p(256)


def _sweep(L, conf=P, idx_a=P, idx_b=P, Q=10, m=5, la=P, Nka=20, lb=P, Nkb=30, ql=P, nl=4, seg=None, nseg=1, thr=P, T=1000, ks=(1, 3, 5), hits=P, err=P,
           ws=P, ws_bytes=1 << 20):
    return L.clibd_threshold_sweep_hits(conf, idx_a, idx_b, Q, m, la, Nka, lb, Nkb, ql, nl, seg, nseg, thr, T, None if ks is None else _arr(ks),
                                        0 if ks is None else len(ks), hits, err, ws, ws_bytes, None)


def test_sweep_validation_needs_no_gpu(lib):
    L = lib
    for name in ("conf", "idx_a", "idx_b", "la", "lb", "ql", "thr", "hits", "err", "ws"):
        assert _sweep(L, **{name: None}) == -1 and b"null" in L.clibd_last_error(), name
    assert _sweep(L, ks=None) == -1 and b"null" in L.clibd_last_error()
    assert _sweep(L, Q=0) == -1 and _sweep(L, Nka=0) == -1 and _sweep(L, Nkb=0) == -1
    assert _sweep(L, m=0) == -1 and b"m <= 8" in L.clibd_last_error()
    assert _sweep(L, m=9, ks=(1,)) == -1 and b"m <= 8" in L.clibd_last_error()
    assert _sweep(L, nl=0) == -1 and _sweep(L, nl=9) == -1 and b"L <= 8" in L.clibd_last_error()
    assert _sweep(L, m=8, ks=tuple(range(1, 10))) == -1 and b"n_k" in L.clibd_last_error()
    assert _sweep(L, ks=(1, 3, 6)) == -1 and b"k <= m" in L.clibd_last_error()
    assert _sweep(L, ks=(0, 1)) == -1
    assert _sweep(L, ks=(1, 5, 3)) == -1 and b"ascending" in L.clibd_last_error()
    assert _sweep(L, ks=(1, 1)) == -1 and b"ascending" in L.clibd_last_error()
    assert _sweep(L, T=0) == -1 and b"T >= 1" in L.clibd_last_error()
    assert _sweep(L, nseg=2) == -1 and b"nseg" in L.clibd_last_error()                  # two segments need a segment array
    assert _sweep(L, nseg=65, seg=P) == -1
    assert _sweep(L, T=(1 << 31) // (64 * 8 * 8), m=8, nl=8, ks=tuple(range(1, 9)), nseg=64, seg=P) == -1 and b"2^31" in L.clibd_last_error()
    assert _sweep(L, ws_bytes=10 * 4 * 4 - 1) == -1 and b"workspace" in L.clibd_last_error()
    assert _sweep(L, ws=ctypes.c_void_p(260)) == -1 and b"workspace" in L.clibd_last_error()
    assert L.clibd_threshold_sweep_workspace_bytes(10, 4) == 160 and L.clibd_threshold_sweep_workspace_bytes(16000, 4) == 256000
    assert L.clibd_threshold_sweep_workspace_bytes(0, 4) == 0 and L.clibd_threshold_sweep_workspace_bytes(10, 9) == 0


def test_merge_validation_needs_no_gpu(lib):
    L = lib

    def merge(conf=P, idx_a=P, idx_b=P, Q=10, m=5, Nka=20, Nkb=30, thr=0.5, merged=P, from_a=P, err=P):
        return L.clibd_threshold_merge(conf, idx_a, idx_b, Q, m, Nka, Nkb, thr, merged, from_a, err, None)

    for name in ("conf", "idx_a", "idx_b", "merged", "from_a", "err"):
        assert merge(**{name: None}) == -1 and b"null" in L.clibd_last_error(), name
    assert merge(Q=0) == -1 and merge(Nka=0) == -1 and merge(Nkb=0) == -1
    assert merge(m=0) == -1 and merge(m=9) == -1 and b"m <= 8" in L.clibd_last_error()
    assert merge(Q=(1 << 31) // 8, m=8) == -1 and b"2^31" in L.clibd_last_error()


def test_wrappers_refuse_host_tensors():
    from clibd_amd import ops

    c, i = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64)
    lab = torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.threshold_sweep_hits(c, i, i, lab, lab, lab[:2], torch.zeros(5, dtype=torch.float64), [1])
    with pytest.raises(ValueError):
        ops.threshold_merge(c, i, i, 4, 4, 0.5)
