"""GPU checks of the SimCLR pre-training path: the fused NT-Xent loss (csrc/ntxent.hip) against the fp64 restatement of
tests/test_simclr_cpu.py, Adam with coupled L2 against torch.optim.Adam, one SimCLR step against the CPU oracle, and the checkpoint
round trip into `load_clip_model`.  Tolerances of the loss are the project's own for the same split-bf16 operand technique
(tests/test_ops_gpu.py::test_softce_rows_fwd_bwd): |loss - ref| < 2e-4 |ref| + 1e-3, rel_err(df, ref) < 1e-4."""
import functools
import types

import pytest
import torch

from tests.test_simclr_cpu import ntxent_fp64_grad, top1_hits_fp64

pytestmark = pytest.mark.gpu

TAU = 0.07


def rel_err(a, b):      # as in tests/test_ops_gpu.py
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def loss_close(got, ref):
    return abs(got - ref) < 2e-4 * abs(ref) + 1e-3


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


@functools.lru_cache(maxsize=None)
def case(b, D, seed=0):
    """(features fp32 [2b, D] = randn * 3, un-normalised; fp64 loss; fp64 gradient; fp64 logits; partner index), computed once per shape"""
    f = torch.randn(2 * b, D, generator=torch.Generator().manual_seed(1000 * b + D + seed)) * 3
    loss, df, s, partner = ntxent_fp64_grad(f, TAU)
    return f, loss.item(), df, s, partner


def run(ops, dev, f, tau=TAU, dloss=None, backward=True):
    fd = f.to(dev).contiguous()
    ws = ops.ntxent_workspace(fd.shape[0], fd.shape[1], dev)
    loss = torch.full((1,), float("nan"), device=dev)
    top1 = torch.full((1,), -1, dtype=torch.int32, device=dev)
    ops.ntxent_fwd(fd, 1.0 / tau, loss, ws, top1)
    df = None
    if backward:
        df = torch.full_like(fd, float("nan"))
        ops.ntxent_bwd(fd, 1.0 / tau, df, ws, None if dloss is None else torch.tensor([dloss], device=dev))
    torch.cuda.synchronize()
    return loss.item(), int(top1.item()), None if df is None else df.cpu()


# (2, 1000): N = 4, the minimum; (3, 1000): odd half, the partner index wraps; (33, 1000): N = 66 crosses a 64-row block, the partner in another
# block; (64, 768): exact tiles; (100, 1000): ragged last tile; (500, 1000): the reference's batch
@pytest.mark.parametrize("b,D", [(2, 1000), (3, 1000), (8, 64), (33, 1000), (64, 768), (100, 1000), (500, 1000)])
def test_ntxent_fwd_bwd_against_fp64(ops, dev, b, D):
    f, ref_loss, ref_df, _, _ = case(b, D)
    loss, _, df = run(ops, dev, f)
    print(f"b={b} D={D}: loss {loss:.7f} ref {ref_loss:.7f}, rel_err(df) {rel_err(df, ref_df):.3e}")
    assert loss_close(loss, ref_loss), (loss, ref_loss)
    assert rel_err(df, ref_df) < 1e-4, rel_err(df, ref_df)
    # an upstream gradient scales the result: the same product with one more fp32 factor, a few ulp per element
    loss2, _, df2 = run(ops, dev, f, dloss=0.37)
    assert loss2 == loss
    assert ((df2.double() - 0.37 * df.double()).abs() <= 1e-6 * df.double().abs() + 1e-37).all()
    assert rel_err(df2, 0.37 * ref_df) < 1e-4


def _natural_scale(f, tau):
    """the size of one term of the feature gradient: (1 / tau) * |W_ij| <= 2 / N, times the largest inverse row norm"""
    n = f.shape[0]
    return (1.0 / tau) * (2.0 / n) / f.double().norm(dim=1).min().item()


@pytest.mark.parametrize("tau", [0.07, 0.01])
def test_ntxent_identical_views(ops, dev, tau):
    """f[i + b] = f[i]: the positive logit is the row maximum 1 / tau and every row is a top-1 hit; at tau = 0.01 the logits reach 100 and
    exp overflows fp32 without the running maximum.  The reference gradient is a difference of terms that cancel (softmax ~ one-hot: 1e-5 of
    the terms' size at tau = 0.07, e^-80 at 0.01), so it is compared in absolute terms, 1e-4 of one term's size (_natural_scale)."""
    b, D = 33, 1000
    half = torch.randn(b, D, generator=torch.Generator().manual_seed(7)) * 3
    f = torch.cat([half, half])
    ref_loss, ref_df, s, partner = ntxent_fp64_grad(f, tau)
    n = 2 * b
    assert torch.allclose(s[torch.arange(n), partner], torch.full((n,), 1.0 / tau, dtype=torch.float64), rtol=1e-12)
    loss, top1, df = run(ops, dev, f, tau=tau)
    print(f"tau={tau}: loss {loss:.3e} ref {ref_loss.item():.3e}, max |df - ref| {(df.double() - ref_df).abs().max().item():.3e}, "
          f"bound {1e-4 * _natural_scale(f, tau):.3e}")
    assert torch.isfinite(df).all() and loss == loss and abs(loss) != float("inf")
    assert loss_close(loss, ref_loss.item()), (loss, ref_loss.item())
    assert top1 == n
    assert (df.double() - ref_df).abs().max().item() < 1e-4 * _natural_scale(f, tau)


def test_ntxent_all_rows_equal(ops, dev):
    """every logit equal: loss = log(N - 1) exactly when the diagonal is removed (log N otherwise), and the gradient vanishes"""
    import math

    n, D = 66, 1000
    row = torch.randn(1, D, generator=torch.Generator().manual_seed(8)) * 3
    f = row.repeat(n, 1)
    loss, _, df = run(ops, dev, f)
    assert abs(loss - math.log(n - 1)) < 1e-4, (loss, math.log(n - 1))
    assert df.abs().max().item() < 1e-4


def test_ntxent_zero_row_follows_normalize_eps(ops, dev):
    """one all-zero feature row: F.normalize divides by max(norm, 1e-12), so the row stays zero and its gradient is g / 1e-12 — finite"""
    f, _, _, _, _ = case(33, 1000)
    f = f.clone()
    f[5] = 0
    ref_loss, ref_df, _, _ = ntxent_fp64_grad(f, TAU)
    assert torch.isfinite(ref_df).all()
    loss, _, df = run(ops, dev, f)
    assert torch.isfinite(df).all()
    assert loss_close(loss, ref_loss.item()), (loss, ref_loss.item())
    keep = torch.arange(f.shape[0]) != 5
    assert rel_err(df[5], ref_df[5]) < 1e-4 and rel_err(df[keep], ref_df[keep]) < 1e-4, (rel_err(df[5], ref_df[5]), rel_err(df[keep], ref_df[keep]))


@pytest.mark.parametrize("b,D", [(33, 1000), (100, 1000)])
def test_ntxent_top1_hits(ops, dev, b, D):
    f, _, _, s, partner = case(b, D)
    hits, margin = top1_hits_fp64(s, partner)
    assert margin > 1e-3, margin          # no comparison within rounding distance: the count is exact
    _, top1, _ = run(ops, dev, f, backward=False)
    assert top1 == hits, (top1, hits)


def test_ntxent_is_bit_reproducible(ops, dev):
    f, _, _, _, _ = case(100, 1000)
    l1, t1, d1 = run(ops, dev, f)
    l2, t2, d2 = run(ops, dev, f)
    assert l1 == l2 and t1 == t2 and torch.equal(d1, d2)


def test_ntxent_loss_module_autograd(dev):
    from clibd_amd.simclr import NTXentLoss

    f, ref_loss, ref_df, s, partner = case(33, 1000)
    crit = NTXentLoss(TAU)
    x = f.to(dev).requires_grad_(True)
    loss = crit(x)
    other = crit(x.detach() * 2 + 1)          # a second forward on the same workspace before the first one's backward
    (loss * 0.5).backward()
    assert loss_close(loss.item(), ref_loss) and other.item() == other.item()
    assert rel_err(x.grad.cpu(), 0.5 * ref_df) < 1e-4


# ------------------------------------------------------------------------------------------ optimizer
def test_adam_l2_matches_torch_adam(ops, dev):
    g = torch.Generator().manual_seed(16)
    n = 10007
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(3)]
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step, gr in enumerate(grads, 1):
        pt.grad = gr.clone()
        opt.step()
        ops.adam_l2_step(p, (gr * 4).to(dev), m, v, 3e-3, 0.9, 0.999, 1e-8, 1e-4, step, grad_scale=0.25)
    torch.cuda.synchronize()
    assert (p.cpu() - pt.detach()).abs().max().item() < 2e-6


def test_fused_adam_under_cosine_annealing_and_not_adamw(dev):
    from torch.optim import lr_scheduler

    from clibd_amd.optim import FusedAdam, FusedAdamW

    g = torch.Generator().manual_seed(41)
    shapes = [(4, 768), (768, 4), (768, 768), (768,), ()]
    init = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    mine = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    fo, ro = FusedAdam(mine, lr=3e-4, weight_decay=1e-4), torch.optim.Adam(ref, lr=3e-4, weight_decay=1e-4)
    fs, rs = lr_scheduler.CosineAnnealingLR(fo, T_max=10, eta_min=0), lr_scheduler.CosineAnnealingLR(ro, T_max=10, eta_min=0)
    for _ in range(10):
        fo.zero_grad()
        ro.zero_grad()
        for a, b in zip(mine, ref):
            gr = torch.randn(a.shape, generator=g)
            a.grad.copy_(gr.to(dev))
            b.grad = gr.clone()
        fo.step(); ro.step(); fs.step(); rs.step()
        assert fo.param_groups[0]["lr"] == ro.param_groups[0]["lr"]
    torch.cuda.synchronize()
    for a, b in zip(mine, ref):
        assert (a.detach().cpu() - b.detach()).abs().max().item() < 5e-6
    # coupled L2 is not decoupled decay: the same gradients through FusedAdamW end elsewhere
    pa, pw = torch.nn.Parameter(init[2].clone().to(dev)), torch.nn.Parameter(init[2].clone().to(dev))
    oa, ow = FusedAdam([pa], lr=1e-2, weight_decay=0.1), FusedAdamW([pw], lr=1e-2, weight_decay=0.1)
    gr = torch.randn(init[2].shape, generator=g).to(dev)
    for o, p in ((oa, pa), (ow, pw)):
        o.zero_grad()
        p.grad.copy_(gr)
        o.step()
    assert (pa.detach() - pw.detach()).abs().max().item() > 1e-4


# ------------------------------------------------------------------------------------------ the step and the checkpoint
def _args(**image):
    mc = types.SimpleNamespace(temperature=TAU, n_views=2, batch_size=4, epochs=1, model_output_name="simclr_test", output_dim=768,
                               disable_lora=True, image=types.SimpleNamespace(**image))
    return types.SimpleNamespace(model_config=mc, project_root_path=".")


def _views(g, b=4):
    """Two views of b structured images: a per-image colour shared by both views plus per-view 16 x 16 colour blocks.  Uniform-noise images
    leave the eight features of a randomly initialised ViT parallel within cos 0.997, and the loss then depends on differences at the size
    of the bf16 rounding: the oracle's own gradients move by 7-11 % between its fp32 and bf16 modes there, by 1 % on these images."""
    col = torch.rand(b, 3, 1, 1, generator=g)

    def view():
        blocks = torch.rand(b, 3, 14, 14, generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)
        return 0.5 * blocks + 0.5 * col

    return view(), view()


def test_simclr_step_matches_oracle(dev):
    """One SimCLR step on a two-block ViT-S-wide tower (384, 6 heads: the narrowest shape of tests/test_model_gpu.py::test_other_vit_sizes_match_oracle),
    b = 4, two views, 1000-wide head, against the CPU oracle with the kernels' bf16 rounding points plus the fp64 loss under autograd.  Gates of
    tests/test_model_gpu.py::test_image_tower_full_finetune_gradients for the same tensors: gradients rel < 3e-2 and cosine > 0.999; the loss
    within 1e-3 (that file's gate for losses against the bf16-emulating oracle); the un-normalised head outputs within 6e-3, the gate
    test_other_vit_sizes_match_oracle puts on them at this width."""
    from oracle import clibd_oracle as O
    from clibd_amd.model import create_vit
    from clibd_amd.optim import FusedAdam
    from clibd_amd.simclr import SimCLR, SimCLRViT
    from tests.test_simclr_cpu import ntxent_fp64

    torch.manual_seed(3)
    om = O.VisionTransformer(img_size=224, patch=16, dim=384, depth=2, heads=6, num_classes=1000)
    vit = create_vit("vit_small_patch16_224", num_classes=1000, depth=2)
    vit.load_state_dict(om.state_dict(), strict=True)
    model = SimCLRViT(vit).to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    v1, v2 = _views(torch.Generator().manual_seed(4))

    names = ["head.weight", "blocks.0.attn.qkv.weight", "patch_embed.proj.weight", "pos_embed"]
    with O.precision("bf16"):
        yo = om(torch.cat([v1, v2]))
        lo, _, _ = ntxent_fp64(yo, TAU)
        ops_ = dict(om.named_parameters())
        go = dict(zip(ops_, torch.autograd.grad(lo, list(ops_.values()))))

    # Adam's first step is lr * g / (|g| + eps): at the default eps = 1e-8 a sign function, which turns any gradient error near zero into 2 lr.
    # eps = 1 keeps the update linear in the gradient, so the gradient gates carry over to the update (times lr).
    lr, eps, wd = 1e-2, 1.0, 1e-4
    ref_params = {n: torch.nn.Parameter(p.detach().clone()) for n, p in om.named_parameters()}
    ro = torch.optim.Adam(list(ref_params.values()), lr=lr, eps=eps, weight_decay=wd)
    for n, p in ref_params.items():
        p.grad = go[n].float().clone()
    ro.step()

    opt = FusedAdam(model.parameters(), lr=lr, eps=eps, weight_decay=wd)
    sim = SimCLR(model=model, optimizer=opt, scheduler=None, device=dev, args=_args())
    before = {n: p.detach().cpu().clone() for n, p in vit.named_parameters()}
    with torch.no_grad():
        y = model(torch.cat([v1, v2]).to(dev))
    loss = sim.train_step(v1, v2)
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu().clone() for n, p in vit.named_parameters()}

    rel = rel_err
    cos = lambda a, b: (a.double().flatten() @ b.double().flatten() / (a.double().norm() * b.double().norm() + 1e-30)).item()
    print(f"features rel {rel(y.cpu(), yo.detach()):.3e}; loss {loss.item():.6f} oracle {lo.item():.6f}")
    assert rel(y.cpu(), yo.detach()) < 6e-3
    assert abs(loss.item() - lo.item()) < 1e-3, (loss.item(), lo.item())
    for n in names:
        print(f"{n}: grad rel {rel(got[n], go[n]):.3e} cos {cos(got[n], go[n]):.6f}")
        assert rel(got[n], go[n]) < 3e-2 and cos(got[n], go[n]) > 0.999, (n, rel(got[n], go[n]), cos(got[n], go[n]))
    after = {n: p.detach().cpu() for n, p in vit.named_parameters()}
    for n in names:
        d_got, d_ref = after[n] - before[n], ref_params[n].detach() - before[n]
        assert d_ref.abs().max().item() > 0
        assert rel(d_got, d_ref) < 3e-2, (n, rel(d_got, d_ref))       # the gradient gate, times lr on both sides


def test_simclr_checkpoint_round_trip(dev, tmp_path):
    from torch.optim import lr_scheduler

    from clibd_amd.model import load_clip_model
    from clibd_amd.optim import FusedAdam
    from clibd_amd.simclr import SimCLR, load_vit_for_simclr_training

    torch.manual_seed(5)
    args = _args(pre_train_model="vit_small_patch16_224")
    model = load_vit_for_simclr_training(args, device=dev)
    assert all(p.requires_grad for p in model.parameters())
    opt = FusedAdam(model.parameters(), lr=3e-4, weight_decay=1e-4)
    sim = SimCLR(model=model, optimizer=opt, scheduler=lr_scheduler.CosineAnnealingLR(opt, T_max=2), device=dev, args=args)
    g = torch.Generator().manual_seed(6)
    loader = [(torch.rand(4, 3, 224, 224, generator=g), torch.rand(4, 3, 224, 224, generator=g)) for _ in range(2)]
    w0 = model.module.blocks[0].mlp.fc1.weight.detach().clone()
    best = sim.train(loader, rank=0, ckpt_dir=str(tmp_path))
    assert best == best and (model.module.blocks[0].mlp.fc1.weight.detach() - w0).abs().max().item() > 0
    assert (tmp_path / "checkpoint_0001.pth.tar").exists()
    ck = torch.load(tmp_path / "model_best.pth.tar", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["arch", "epoch", "optimizer", "state_dict"] and ck["arch"] == "vit_small_patch16_224"
    sd = ck["state_dict"]
    assert sd and all(k.startswith("module.") for k in sd)

    # the consumer: load_clip_model's strict load of the SimCLR-style file
    cargs = _args(pre_train_model="vit_small_patch16_224", image_encoder_trained_with_simclr_style_ckpt_path=str(tmp_path / "model_best.pth.tar"))
    clip = load_clip_model(cargs, device=None)
    loaded = {k.replace(".attn.qkv.qkv.", ".attn.qkv."): v for k, v in clip.image_encoder.base_image_encoder.state_dict().items() if ".linear_" not in k}
    trained = {k: v.detach().cpu() for k, v in model.module.state_dict().items()}
    assert sorted(loaded) == sorted(trained)
    for k, v in trained.items():
        if not k.startswith("head."):           # the CLIP tower replaces the classifier by its own projection
            assert torch.equal(loaded[k], v), k

    # the other direction: a file written the reference's way loads into the training model
    plain = {k: torch.randn(v.shape, generator=g) for k, v in trained.items()}
    path = tmp_path / "reference_style.pth.tar"
    torch.save({"state_dict": {"module." + k: v for k, v in plain.items()}}, path)
    fresh = load_vit_for_simclr_training(args)
    fresh.load_state_dict(torch.load(path, map_location="cpu", weights_only=False)["state_dict"], strict=True)
    for k, v in fresh.module.state_dict().items():
        assert torch.equal(v, plain[k]), k
