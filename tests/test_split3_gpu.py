"""The split-bf16 product module (csrc/split3.hip) at its edges, reached through both of its callers: K9's loss (clibd_softce_rows_fwd /
_bwd) and the linear-probe head (clibd_linear_f32_fwd / _bwd), against fp64 references computed here.  The shapes are the smallest at
which a padding or a segment order can go wrong (D = 64: D must be a multiple of 64):
  loss (Nx, N, row0) = (1, 17, 16): one row, N padded 17 -> 32 rows and 17 -> 64 along the contraction, a non-zero row offset;
       (65, 65, 0): both contractions cross one 64 tile by a single element;
  head (B, C, D) = (1, 1, 64); (65, 17, 64); (3, 65, 128) without a bias, and with only dx and only dw requested.
None of them is among the shapes of tests/test_ops_gpu.py::test_softce_rows_fwd_bwd (all at D = 768) or of
tests/test_method_linear_gpu.py::test_kernels_against_fp64, so none was dropped.  The gates are those two tests' for the same quantities:
|loss - ref| < 2e-4 |ref| + 1e-3, rel_err < 1e-4 for dx, dy (logits, dx, dw, db), |dscale - ref| < 1e-3 |ref| + 1e-6.  Every sum has one
order, so a second call returns the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


def rel_err(a, b):      # as in tests/test_ops_gpu.py
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _loss_case(ops, dev, x, y, labels, row0, scale, w, dy0):
    Nx, D = x.shape
    N = y.shape[0]
    ws = ops.softce_workspace(Nx, N, D, dev)
    loss = torch.zeros(1, device=dev)
    sc = torch.tensor([scale], device=dev)
    ops.softce_rows_fwd(x.to(dev), y.to(dev), labels.to(dev), row0, sc, loss, ws)
    dx, dy, ds = torch.zeros((Nx, D), device=dev), dy0.to(dev), torch.zeros(1, device=dev)
    ops.softce_rows_bwd(labels.to(dev), Nx, N, D, row0, sc, w, dx, dy, ds, ws)
    torch.cuda.synchronize()
    return loss.cpu(), dx.cpu(), dy.cpu(), ds.cpu()


def _check_loss(ops, dev, Nx, N, row0):
    g = torch.Generator().manual_seed(1000 * N + Nx)
    D = 64
    x = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)[row0 : row0 + Nx].contiguous()
    y = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    labels = torch.arange(N) // 2      # pairs share a label; the last row of an odd N is alone
    scale = 1.0 / 0.07
    xd, yd = x.double().requires_grad_(True), y.double().requires_grad_(True)
    sd = torch.tensor(scale, dtype=torch.float64, requires_grad=True)
    S = sd * (xd @ yd.T)
    T = (labels[row0 : row0 + Nx, None] == labels[None, :]).to(S.dtype)
    ref = -(T * torch.log_softmax(S, dim=1)).sum()
    w = 0.37 / N
    gx, gy, gs = torch.autograd.grad(ref * w, (xd, yd, sd))
    dy0 = torch.randn(N, D, generator=g) * float(gy.abs().mean())      # accumulate semantics, as in test_softce_rows_fwd_bwd
    loss, dx, dy, ds = _loss_case(ops, dev, x, y, labels, row0, scale, w, dy0)
    print(f"(Nx, N, row0) = ({Nx}, {N}, {row0}): loss {loss.item():.7f} ref {ref.item():.7f}, rel_err dx {rel_err(dx, gx):.2e} "
          f"dy {rel_err(dy - dy0, gy):.2e}, dscale {ds.item():.7e} ref {gs.item():.7e}")
    assert abs(loss.item() - ref.item()) < 2e-4 * abs(ref.item()) + 1e-3
    assert rel_err(dx, gx) < 1e-4
    assert rel_err(dy - dy0, gy) < 1e-4
    assert abs(ds.item() - gs.item()) < 1e-3 * abs(gs.item()) + 1e-6
    again = _loss_case(ops, dev, x, y, labels, row0, scale, w, dy0)
    assert all(torch.equal(a, b) for a, b in zip((loss, dx, dy, ds), again))


def _check_head(ops, dev, B, C, D, bias):
    g = torch.Generator().manual_seed(100000 * B + 100 * C + D)
    x = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=-1)
    w = torch.randn(C, D, generator=g) * 3.0      # unit rows: logits ~ N(0, 3^2), as in tests/test_method_linear_gpu.py
    b = torch.randn(C, generator=g) * 0.5 if bias else None
    dout = torch.randn(B, C, generator=g) / B
    ref = dict(logits=x.double() @ w.double().T + (b.double() if bias else 0.0), dx=dout.double() @ w.double(), dw=dout.double().T @ x.double(),
               db=dout.double().sum(0))
    xd, wd, dd = x.to(dev), w.to(dev), dout.to(dev)
    bd = b.to(dev) if bias else None

    def run(**need):
        logits = ops.linear_f32_fwd(xd, wd, bd)
        dx, dw, db = ops.linear_f32_bwd(dd, xd, wd, **need)
        torch.cuda.synchronize()
        return dict(logits=logits.cpu(), dx=None if dx is None else dx.cpu(), dw=None if dw is None else dw.cpu(),
                    db=None if db is None else db.cpu())

    got = run()
    print(f"(B, C, D) = ({B}, {C}, {D}): " + ", ".join(f"rel_err {n} {rel_err(got[n], ref[n]):.2e}" for n in ("logits", "dx", "dw", "db")))
    for name in ("logits", "dx", "dw", "db"):
        assert rel_err(got[name], ref[name]) < 1e-4, (name, rel_err(got[name], ref[name]))
    again = run()
    assert all(torch.equal(got[n], again[n]) for n in got)
    if not bias:      # each product alone skips the other's operand images: the same bits as together
        only_dx = run(need_dw=False, need_db=False)
        only_dw = run(need_dx=False, need_db=False)
        assert only_dx["dw"] is None and only_dx["db"] is None and torch.equal(only_dx["dx"], got["dx"])
        assert only_dw["dx"] is None and only_dw["db"] is None and torch.equal(only_dw["dw"], got["dw"])


@pytest.mark.parametrize("path,case", [("loss", (1, 17, 16)), ("loss", (65, 65, 0)), ("head", (1, 1, 64, True)), ("head", (65, 17, 64, True)),
                                       ("head", (3, 65, 128, False))])
def test_split3_module_edges(ops, dev, path, case):
    (_check_loss if path == "loss" else _check_head)(ops, dev, *case)
