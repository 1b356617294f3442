"""CPU checks of the SimCLR additions: the second header (include/clibd_hip_simclr.h) and its binding table, host-side validation of the
NT-Xent entries, the workspace's O(N * D) growth, the test-side fp64 restatement of the loss against numbers generated from the reference
(tests/golden/simclr_golden.pt, tools/make_simclr_golden.py), and the new unit's scratch-free register budget."""
import ctypes
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "clibd_hip_simclr.h"
GOLDEN = ROOT / "tests" / "golden" / "simclr_golden.pt"


def ntxent_fp64(f: torch.Tensor, temperature: float):
    """NT-Xent over [2b, D] features in fp64: loss, the masked logits S (diagonal = -inf) and the partner index of every row.
    Rows i and i + b are the two views of sample i; every row's positive is its partner, every other row but itself a negative."""
    f = f.double()
    n = f.shape[0]
    fh = torch.nn.functional.normalize(f, dim=1, eps=1e-12)
    s = (fh @ fh.T) / temperature
    s = s.masked_fill(torch.eye(n, dtype=torch.bool), float("-inf"))
    partner = (torch.arange(n) + n // 2) % n
    loss = (torch.logsumexp(s, dim=1) - s[torch.arange(n), partner]).mean()
    return loss, s, partner


def ntxent_fp64_grad(f: torch.Tensor, temperature: float):
    x = f.double().clone().requires_grad_(True)
    loss, s, partner = ntxent_fp64(x, temperature)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g, s.detach(), partner


def top1_hits_fp64(s: torch.Tensor, partner: torch.Tensor):
    """(hit count, smallest |positive - best negative| over the rows) from the fp64 logits"""
    n = s.shape[0]
    pos = s[torch.arange(n), partner]
    neg = s.clone()
    neg[torch.arange(n), partner] = float("-inf")
    best = neg.max(dim=1).values
    return int((pos >= best).sum()), float((pos - best).abs().min())


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


def test_simclr_header_says_the_abi_stays_and_its_unit_is_built():
    from clibd_amd import build

    assert "stays 7" in HEADER.read_text().split("*/")[0]      # the opening comment says that the ABI version does not move
    assert HEADER in build._deps() and "ntxent" in build.SOURCES


def test_ntxent_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    need = L.clibd_ntxent_workspace_bytes(8, 1000)
    assert need > 0

    def fwd(f=P(256), N=8, D=1000, loss=P(256), ws=P(4096), nbytes=need):
        return L.clibd_ntxent_fwd(f, N, D, 1 / 0.07, loss, None, ws, nbytes, None)

    def bwd(f=P(256), N=8, D=1000, df=P(256), ws=P(4096), nbytes=need):
        return L.clibd_ntxent_bwd(f, N, D, 1 / 0.07, None, df, ws, nbytes, None)

    for call in (fwd, bwd):
        for kw, word in ((dict(N=7), b"even"), (dict(N=2), b"at least 4"), (dict(D=0), b"D must"), (dict(f=None), b"null"),
                         (dict(ws=None), b"null workspace"), (dict(nbytes=need - 1), b"too small"), (dict(ws=P(4096 + 8)), b"aligned")):
            assert call(**kw) == -1, kw
            assert word in L.clibd_last_error(), (kw, L.clibd_last_error())
    assert fwd(loss=None) == -1 and b"null loss" in L.clibd_last_error()
    assert bwd(df=None) == -1 and b"null gradient" in L.clibd_last_error()
    assert L.clibd_adam_l2_step(None, None, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) == -1
    assert L.clibd_adam_l2_step(P(16), P(16), P(16), P(16), 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, None) == -1
    assert b"step" in L.clibd_last_error()


def test_ntxent_workspace_holds_no_square_matrix(lib):
    from clibd_amd import _lib

    L = _lib.load()
    ws = L.clibd_ntxent_workspace_bytes
    assert 0 < ws(4096, 1000) < 4096 * 4096 * 4
    assert ws(4096, 1000) <= 2.2 * ws(2048, 1000)
    assert ws(4, 1) > 0 and ws(0, 8) == 0 and ws(8, 0) == 0


def test_fp64_restatement_reproduces_the_reference_numbers():
    """The golden file holds the reference's own info_nce_loss + CrossEntropyLoss in fp32 on the CPU; the restatement above is evaluated
    in fp64, so the differences are the fp32 evaluation's error: loss 1e-6, gradients 1e-5 relative."""
    g = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    assert [(c["b"], c["D"]) for c in g["cases"]] == [(4, 1000), (16, 768)] and g["temperature"] == 0.07
    for c in g["cases"]:
        f = c["features"]
        assert f.dtype == torch.float32 and tuple(f.shape) == (2 * c["b"], c["D"])
        loss, df, s, partner = ntxent_fp64_grad(f, g["temperature"])
        assert abs(loss.item() - c["loss"].double().item()) < 1e-6 * abs(loss.item()), (loss.item(), c["loss"].item())
        rel = ((df - c["dfeatures"].double()).norm() / df.norm()).item()
        assert rel < 1e-5, rel
        hits, margin = top1_hits_fp64(s, partner)
        assert margin > 1e-3 and hits == c["top1_hits"]


def test_not_supported_views_and_shapes_raise_on_the_host():
    from clibd_amd.engine import NotSupportedYet
    from clibd_amd.simclr import NTXentLoss

    with pytest.raises(NotSupportedYet):
        NTXentLoss(0.07, n_views=3)
    with pytest.raises(ValueError):
        NTXentLoss(0.07)(torch.zeros(3, 8))
    with pytest.raises(ValueError):
        NTXentLoss(0.0)


def test_ntxent_unit_uses_no_scratch():
    """Every kernel of csrc/ntxent.hip keeps its working set in registers (the parse of tests/test_abi.py::test_hot_kernels_use_no_scratch)."""
    from clibd_amd import build

    rows = [(k["name"], k["scratch"]) for k in build.resource_usage("ntxent")]
    names = " ".join(n for n, _ in rows)
    for k in ("ntxent_prep_kernel", "ntxent_fwd_kernel", "ntxent_reduce_kernel", "ntxent_transpose_kernel", "ntxent_bwd_kernel", "ntxent_bwd_rows_kernel"):
        assert k in names, (k, names)
    assert not [(n, s) for n, s in rows if s > 0], rows
