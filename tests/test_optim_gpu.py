"""GPU checks of the optimizer's clipping, parameter groups and non-finite skip (clibd_amd.optim, include/clibd_hip_optim.h).

Norm: against the fp64 restatement of tests/optim_reference.py; the gate on the relative error is 3 x the error of the fp32 restatement
(the kernel's documented order) against fp64, with a floor of 2^-22.  Update: bit for bit against the existing kernels wherever the
arithmetic is the same (inactive clipping, every group's slice, the drivers' step), and against torch.optim.AdamW / Adam with
clip_grad_norm_ in fp64, gated by 3 x the error of the same torch recipe in fp32 (floor 5e-6, the gate of
tests/test_ops_gpu.py::test_fused_adamw_under_one_cycle_lr_on_the_gpu).  Every figure is printed before it is asserted.

Measured on an MI355X: see DESIGN §3.17."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import optim_reference as OR  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32


def pad64(n):
    return (n + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def norm_case(n):
    """(gradient, {grad_scale: (fp64 norm, gate, fp32 restatement's error)}): computed once, shared, never written"""
    g = OR.gradient(n)
    g.setflags(write=False)
    return g, {gs: OR.norm_gate(g, gs) for gs in (1.0, 0.25)}


def run_norm(ops, g, grad_scale=1.0, max_norm=None, skip=False, record=None):
    """the norm launch with the workspace inside a poisoned buffer: (record on the CPU, float view, workspace tail intact)"""
    dev = g.device
    if record is None:
        record = torch.zeros((4,), dtype=torch.int32, device=dev)
    need = ops.grad_norm_workspace(g.numel(), dev).numel()
    buf = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=dev)
    ops.grad_norm(g, record, buf[:need], grad_scale, max_norm, skip)
    rec = record.cpu()
    chunks = max(1, -(-g.numel() // OR.CHUNK))
    return rec, rec.view(F32), bool((buf[4 * chunks:] == 0xAB).all())


# ---- 1. the norm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("n", OR.NORM_SIZES)
def test_norm_against_fp64(dev, n, grad_scale):
    from clibd_amd import ops

    g_np, gates = norm_case(n)
    ref, gate, err32 = gates[grad_scale]
    g = torch.from_numpy(g_np.copy()).to(dev)
    rec, recf, intact = run_norm(ops, g, grad_scale, max_norm=0.5 * ref)
    got, coef = float(recf[0]), recf[1].item()
    err = abs(got - ref) / ref
    print(f"norm n={n} grad_scale={grad_scale}: kernel {got:.9g}, fp64 {ref:.9g}, rel err {err:.3e}, fp32 restatement {err32:.3e}, gate {gate:.3e}")
    assert intact
    assert err <= gate
    assert coef == float(OR.clip_coef(np.float32(got), 0.5 * ref)) and 0 < coef < 1                 # torch's formula on the kernel's own norm, in fp32
    assert rec[2].item() == 0 and rec[3].item() == 0
    rec2, _, _ = run_norm(ops, g, grad_scale, max_norm=0.5 * ref)                                    # two runs are bit-equal
    assert torch.equal(rec, rec2)
    _, recf3, _ = run_norm(ops, g, grad_scale, max_norm=None)                                        # no max_norm: coefficient 1
    assert recf3[0].item() == got and recf3[1].item() == 1.0
    _, recf4, _ = run_norm(ops, g, grad_scale, max_norm=4.0 * ref + 1e-5)                            # below the bound: exactly 1
    assert recf4[1].item() == 1.0


def test_norm_of_zeros_and_nonfinite_values(dev):
    from clibd_amd import ops

    n = 3 * OR.CHUNK + 5
    z = torch.zeros((n,), dtype=F32, device=dev)
    rec, recf, _ = run_norm(ops, z, 1.0, max_norm=1.0, skip=True)
    print("zeros:", recf[:2].tolist(), rec[2:].tolist())
    assert recf[0].item() == 0.0 and recf[1].item() == 1.0 and rec[2:].tolist() == [0, 0]
    for bad, where in ((float("inf"), 0), (float("-inf"), n - 1), (float("nan"), OR.CHUNK + 17)):
        g = torch.from_numpy(norm_case(n)[0].copy()).to(dev)
        g[where] = bad
        record = torch.zeros((4,), dtype=torch.int32, device=dev)
        rec, recf, _ = run_norm(ops, g, 1.0, max_norm=1.0, skip=True, record=record)
        print(f"{bad} at {where}, skip on:", recf[:2].tolist(), rec[2:].tolist())
        assert not np.isfinite(recf[0].item()) and (np.isnan(recf[0].item()) == np.isnan(bad)) and rec[2:].tolist() == [1, 1]
        want_coef = OR.clip_coef(np.float32(recf[0].item()), 1.0)                       # NaN stays NaN, inf gives 0: torch's clamp
        assert (np.isnan(recf[1].item()) and np.isnan(want_coef)) or recf[1].item() == float(want_coef)
        rec, _, _ = run_norm(ops, g, 1.0, max_norm=1.0, skip=True, record=record)      # the count accumulates over two calls
        assert rec[2:].tolist() == [1, 2]
        rec, recf, _ = run_norm(ops, g, 1.0, max_norm=1.0, skip=False, record=record)  # skip off: the norm is as non-finite, the flag is not set
        assert not np.isfinite(recf[0].item()) and rec[2:].tolist() == [0, 2]
        g[where] = 1.0
        rec, recf, _ = run_norm(ops, g, 1.0, max_norm=1.0, skip=True, record=record)   # a clean gradient clears skip_now, keeps the count
        assert np.isfinite(recf[0].item()) and rec[2:].tolist() == [0, 2]


# ---- 2. inactive equals today, bit for bit ---------------------------------------------------------------------------------------------------
def _state(n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=g) * 0.1).to(dev)
    m = (torch.randn(n, generator=g) * 0.01).to(dev)
    v = (torch.rand(n, generator=g) * 1e-3).to(dev)
    return p, m, v, g


@pytest.mark.parametrize("kind", ["adamw", "adam_l2"])
def test_one_group_and_inactive_clipping_equal_the_plain_kernel(dev, kind):
    from clibd_amd import ops

    plain, grouped = (ops.adamw_step, ops.adamw_step_groups) if kind == "adamw" else (ops.adam_l2_step, ops.adam_l2_step_groups)
    n = pad64(10007)
    p, m, v, gen = _state(n, dev, 5)
    a, b, c = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
    record = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = ops.grad_norm_workspace(n, dev)
    lr, wd, gs = 3e-3, 0.05, 0.5
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen).to(dev)
        plain(a[0], g, a[1], a[2], lr, 0.9, 0.999, 1e-8, wd, step, gs)
        ops.grad_norm(g, record, ws, gs, 1e9, True)                                   # a max_norm above the norm: coefficient exactly 1
        grouped(b[0], g, b[1], b[2], [(0, lr, wd)], 0.9, 0.999, 1e-8, step, gs, record)
        grouped(c[0], g, c[1], c[2], [(0, lr, wd)], 0.9, 0.999, 1e-8, step, gs, None)  # no record at all
        coef = record.view(F32)[1].item()
        diffs = [int((x != y).sum()) for x, y in zip(a + a, b + c)]
        print(f"{kind} step {step}: coef {coef}, elements that differ from the plain kernel (p, m, v with record; p, m, v without): {diffs}")
        assert coef == 1.0 and diffs == [0] * 6
    assert not torch.equal(a[0], p)


def test_an_n_that_is_no_multiple_of_four_and_guards(dev):
    """the C entry on an odd length inside poisoned buffers: the last elements take the scalar path, nothing past n is written"""
    from clibd_amd import ops

    n, G = 64 * 3 + 7, 64
    p, m, v, gen = _state(n + 2 * G, dev, 6)
    g = torch.randn(n + 2 * G, generator=gen).to(dev)
    a, b = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
    ops.adamw_step(a[0][G:G + n], g[G:G + n], a[1][G:G + n], a[2][G:G + n], 1e-3, 0.9, 0.999, 1e-8, 0.01, 4, 1.0)
    ops.adamw_step_groups(b[0][G:G + n], g[G:G + n], b[1][G:G + n], b[2][G:G + n], [(0, 1e-3, 0.01)], 0.9, 0.999, 1e-8, 4, 1.0, None)
    for x, y, orig in zip(a, b, (p, m, v)):
        assert torch.equal(x, y) and torch.equal(y[:G], orig[:G]) and torch.equal(y[G + n:], orig[G + n:])
    assert not torch.equal(b[0][G + n - 7:G + n], p[G + n - 7:G + n])


# ---- 3. groups hit the right elements ------------------------------------------------------------------------------------------------------------
GROUP_SHAPES = [[(5, 64)], [(100,), (), (70,)], [(1000,)]]          # group starts 0, 320, 640: 64-float granules, no multiples of 256
GROUP_HYP = [(1e-3, 0.1), (5e-3, 0.0), (2e-4, 0.3)]                  # (lr, weight_decay)


@pytest.mark.parametrize("clip", [None, 1e9])
@pytest.mark.parametrize("kind", ["adamw", "adam_l2"])
def test_every_group_slice_equals_the_plain_kernel_on_that_slice(dev, kind, clip):
    from clibd_amd import ops
    from clibd_amd.optim import FusedAdam, FusedAdamW

    cls, plain = (FusedAdamW, ops.adamw_step) if kind == "adamw" else (FusedAdam, ops.adam_l2_step)
    gen = torch.Generator().manual_seed(9)
    groups = [{"params": [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.1).to(dev)) for s in shapes], "lr": lr, "weight_decay": wd}
              for shapes, (lr, wd) in zip(GROUP_SHAPES, GROUP_HYP)]
    opt = cls(groups, max_grad_norm=clip)
    assert opt._group_first == [0, 320, 640] and opt.flat_p.numel() == 1664 and opt._offsets == [0, 320, 448, 512, 640]
    assert [id(p) for p in opt.bucket_params()] == [id(p) for g in groups for p in g["params"]]
    opt.grad_scale = 0.5
    ref = [opt.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]
    bounds = opt._group_first + [opt.flat_p.numel()]
    for step in (1, 2):
        opt.zero_grad()
        for p in opt.bucket_params():
            p.grad.copy_(torch.randn(p.shape, generator=gen).to(dev))
        g = opt.flat_g.clone()
        opt.step()
        for k, (lr, wd) in enumerate(GROUP_HYP):
            lo, hi = bounds[k], bounds[k + 1]
            plain(ref[0][lo:hi], g[lo:hi], ref[1][lo:hi], ref[2][lo:hi], lr, 0.9, 0.999, 1e-8, wd, step, 0.5)
        for k in range(3):
            lo, hi = bounds[k], bounds[k + 1]
            diffs = [int((x[lo:hi] != y[lo:hi]).sum()) for x, y in zip(ref, (opt.flat_p, opt.exp_avg, opt.exp_avg_sq))]
            print(f"{kind} clip={clip} step {step} group {k} [{lo}, {hi}): elements that differ (p, m, v) {diffs}")
            assert diffs == [0, 0, 0]
    one = opt.bucket_params()[2]
    assert one.numel() == 1 and one.data_ptr() == opt.flat_p.data_ptr() + 4 * 448 and float(one.detach()) == float(opt.flat_p[448])


# ---- 4. against torch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_two_groups_clipped_under_one_cycle_lr_against_torch(dev, kind):
    """the shapes and rates of test_fused_adamw_under_one_cycle_lr_on_the_gpu, split into a decay and a no-decay group, a max_lr per group,
    max_grad_norm = 1 against gradient norms near 770: clipped at every step"""
    from torch.optim import lr_scheduler

    from clibd_amd.optim import FusedAdam, FusedAdamW

    mine_cls, torch_cls = (FusedAdamW, torch.optim.AdamW) if kind == "adamw" else (FusedAdam, torch.optim.Adam)
    gen = torch.Generator().manual_seed(41)
    shapes = [(4, 768), (768, 4), (768, 768), (768,), ()]
    init = [torch.randn(s, generator=gen) * 0.1 for s in shapes]
    lr, max_norm, wd = 1e-3 * 2048 / 500, 1.0, 1e-2
    split = lambda ps: [{"params": ps[:3], "weight_decay": wd}, {"params": ps[3:], "weight_decay": 0.0}]
    mine = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    r64 = [torch.nn.Parameter(t.clone().double()) for t in init]
    r32 = [torch.nn.Parameter(t.clone()) for t in init]
    fo, o64, o32 = mine_cls(split(mine), lr=lr, max_grad_norm=max_norm), torch_cls(split(r64), lr=lr), torch_cls(split(r32), lr=lr)
    mk = lambda o: lr_scheduler.OneCycleLR(o, max_lr=[4 * lr, 2 * lr], total_steps=10, pct_start=0.3, anneal_strategy="cos", cycle_momentum=False)
    fs, s64, s32 = mk(fo), mk(o64), mk(o32)
    for step in range(10):
        fo.zero_grad()
        for a, b, c in zip(mine, r64, r32):
            gr = torch.randn(a.shape, generator=gen)
            a.grad.copy_(gr.to(dev))
            b.grad, c.grad = gr.double(), gr.clone()
        ref, gate, err32 = OR.norm_gate(fo.flat_g.cpu().numpy())
        n64 = float(torch.nn.utils.clip_grad_norm_(r64, max_norm))
        torch.nn.utils.clip_grad_norm_(r32, max_norm)
        fo.step(); o64.step(); o32.step(); fs.step(); s64.step(); s32.step()
        got = fo.grad_norm.item()
        err = abs(got - ref) / ref
        print(f"{kind} step {step}: grad_norm {got:.7g}, fp64 {ref:.7g} (torch fp64 {n64:.7g}), rel err {err:.3e}, gate {gate:.3e}")
        assert got > max_norm and abs(n64 - ref) <= 1e-12 * ref
        assert err <= gate
        assert [g["lr"] for g in fo.param_groups] == [g["lr"] for g in o64.param_groups] and fo.param_groups[0]["lr"] != fo.param_groups[1]["lr"]
    assert int(fo.skipped_steps) == 0
    for i, (a, b, c) in enumerate(zip(mine, r64, r32)):
        e32 = (c.detach().double() - b.detach()).abs().max().item()
        e = (a.detach().cpu().double() - b.detach()).abs().max().item()
        gate = max(3 * e32, 5e-6)
        print(f"{kind} parameter {i} {tuple(a.shape)}: max |fused - fp64| {e:.3e}, max |torch fp32 - fp64| {e32:.3e}, gate {gate:.3e}")
        assert e <= gate
    assert (mine[0].detach().cpu() - init[0]).abs().max().item() > 1e-3


# ---- 5. skip and propagate -----------------------------------------------------------------------------------------------------------------------
def _small(dev, seed, **kw):
    from clibd_amd.optim import FusedAdamW

    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.1).to(dev)) for s in [(300,), (7, 5)]]
    return ps, FusedAdamW(ps, lr=1e-2, **kw)


def _feed(opt, grads):
    opt.zero_grad()
    for p, g in zip(opt.bucket_params(), grads):
        p.grad.copy_(g.to(p.device))


def test_skip_keeps_every_bit_and_counts(dev):
    gen = torch.Generator().manual_seed(2)
    grads = [[torch.randn(s, generator=gen) for s in [(300,), (7, 5)]] for _ in range(3)]
    grads[1][1][3, 2] = float("nan")
    ps, opt = _small(dev, 1, nonfinite="skip")
    _, twin = _small(dev, 1)                                                  # the plain path
    _feed(opt, grads[0]); opt.step()
    _feed(twin, grads[0]); twin.step()
    before = [t.clone() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq)]
    assert torch.equal(opt.flat_p, twin.flat_p) and int(opt.skipped_steps) == 0 and np.isfinite(opt.grad_norm.item())
    _feed(opt, grads[1]); opt.step()
    print("after the poisoned step: grad_norm", opt.grad_norm.item(), "skipped_steps", int(opt.skipped_steps), "step_count", opt.step_count)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, (opt.flat_p, opt.exp_avg, opt.exp_avg_sq)))
    assert int(opt.skipped_steps) == 1 and np.isnan(opt.grad_norm.item()) and opt.step_count == 2
    twin.step_count += 1                                                      # the bias correction counts the skipped step
    _feed(opt, grads[2]); opt.step()
    _feed(twin, grads[2]); twin.step()
    for x, y in ((opt.flat_p, twin.flat_p), (opt.exp_avg, twin.exp_avg), (opt.exp_avg_sq, twin.exp_avg_sq)):
        assert torch.equal(x, y)
    assert int(opt.skipped_steps) == 1 and opt.step_count == twin.step_count == 3 and not torch.equal(opt.flat_p, before[0])
    assert opt.skipped_steps.dtype == torch.int32 and opt.grad_norm.dtype == F32 and opt.grad_norm.is_cuda and opt.skipped_steps.is_cuda


def test_propagate_is_nan_where_torch_is(dev):
    gen = torch.Generator().manual_seed(3)
    grads = [torch.randn(s, generator=gen) for s in [(300,), (7, 5)]]
    grads[0][17] = float("nan")
    for max_norm in (1.0, None):
        ps, opt = _small(dev, 4, max_grad_norm=max_norm, weight_decay=0.0)
        ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
        ro = torch.optim.AdamW(ref, lr=1e-2, weight_decay=0.0)
        for r, g in zip(ref, grads):
            r.grad = g.clone()
        if max_norm:
            torch.nn.utils.clip_grad_norm_(ref, max_norm, error_if_nonfinite=False)
        ro.step()
        _feed(opt, grads); opt.step()
        got = [torch.isnan(p.detach().cpu()) for p in ps]
        want = [torch.isnan(r.detach()) for r in ref]
        print(f"propagate, max_grad_norm={max_norm}: NaN parameters fused {[int(x.sum()) for x in got]}, torch {[int(x.sum()) for x in want]}")
        assert all(torch.equal(x, y) for x, y in zip(got, want)) and int(want[0].sum()) == (300 if max_norm else 1)
        assert int(opt.skipped_steps) == 0


# ---- 6. through the drivers --------------------------------------------------------------------------------------------------------------------
def _pretraining(dev, **opt_kw):
    import mlm_labels_reference as LR
    from test_mlm_gpu import pretraining_model, tied_state

    from clibd_amd.optim import FusedAdamW, decay_parameter_groups

    m = pretraining_model(LR.A, tied_state(55, LR.A), True, dev).eval().set_deterministic(True)      # eval: no dropout draw between the twins
    opt = FusedAdamW(decay_parameter_groups(m, 0.01), lr=1e-3, **opt_kw)
    m.attach(opt)
    return m, opt, LR.A["vocab_size"]


def test_pretrain_step_clips_by_the_norm_of_its_own_gradient(dev):
    from clibd_amd import mlm, ops

    max_norm = 0.05
    m, opt, V = _pretraining(dev, max_grad_norm=max_norm)
    twin, topt, _ = _pretraining(dev, max_grad_norm=max_norm)
    assert len(opt.param_groups) == 2 and [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0] and torch.equal(opt.flat_p, topt.flat_p)
    gen = torch.Generator().manual_seed(8)
    ids = torch.cat([torch.zeros(4, 1, dtype=torch.long), torch.randint(3, V, (4, 16), generator=gen)], dim=1).to(dev)     # B = 4, S = 17
    mlm.pretrain_step(m, ids, opt, mask_ratio=0.5, seed=11)
    topt.zero_grad()                                                           # the twin: forward and backward only
    masked, rows, targets, n_valid = mlm.mask_tokens(ids, 0.5, 11)
    loss, _ = twin(masked, rows, targets, n_valid)
    loss.backward()
    g = topt.flat_g.clone()
    ref, gate, err32 = OR.norm_gate(g.cpu().numpy())
    got, coef = opt.grad_norm.item(), opt._record.view(F32)[1].item()
    err = abs(got - ref) / ref
    print(f"pretrain_step: grad_norm {got:.7g}, fp64 norm of the twin's gradient {ref:.7g}, rel err {err:.3e}, gate {gate:.3e}, coef {coef:.7g}")
    assert err <= gate and coef == float(OR.clip_coef(np.float32(got), max_norm))
    bounds = topt._group_first + [topt.flat_p.numel()]
    for k, grp in enumerate(topt.param_groups):                                # ops.adamw_step per group with grad_scale * coef
        lo, hi = bounds[k], bounds[k + 1]
        ops.adamw_step(topt.flat_p[lo:hi], g[lo:hi], topt.exp_avg[lo:hi], topt.exp_avg_sq[lo:hi], grp["lr"], 0.9, 0.999, grp["eps"], grp["weight_decay"],
                       1, 1.0 * coef)
    diffs = [int((x != y).sum()) for x, y in ((opt.flat_p, topt.flat_p), (opt.exp_avg, topt.exp_avg), (opt.exp_avg_sq, topt.exp_avg_sq))]
    print("elements that differ from the per-group plain update (p, m, v):", diffs, "of", opt.flat_p.numel())
    assert diffs == [0, 0, 0] and int((opt.exp_avg != 0).sum()) > 1000


def test_pretrain_epoch_skips_a_poisoned_batch(dev):
    from clibd_amd import mlm

    m, opt, V = _pretraining(dev, max_grad_norm=1.0, nonfinite="skip")
    gen = torch.Generator().manual_seed(9)
    batches = [torch.cat([torch.zeros(4, 1, dtype=torch.long), torch.randint(3, V, (4, 16), generator=gen)], dim=1).to(dev) for _ in range(2)]
    word = m.bert.embeddings.word_embeddings.weight
    start = opt.flat_p.clone()

    def loader():
        yield batches[0]
        keep = word.detach()[7].clone()
        with torch.no_grad():
            word[7] = float("nan")                                             # NaN embeddings (and, tied, a NaN decoder row) for this batch only
        yield batches[1]
        with torch.no_grad():
            word[7] = keep

    stats = mlm.pretrain_epoch(m, loader(), opt)
    print("pretrain_epoch:", stats, "skipped_steps", int(opt.skipped_steps))
    assert stats["skipped"] == 1 and stats["steps"] == 2 and int(opt.skipped_steps) == 1
    assert bool(torch.isfinite(opt.flat_p).all()) and bool(torch.isfinite(opt.exp_avg).all()) and not torch.equal(opt.flat_p, start)
    stats = mlm.pretrain_epoch(m, batches, opt)                                # the count is per epoch
    assert stats["skipped"] == 0 and int(opt.skipped_steps) == 1 and np.isfinite(stats["loss"])


def test_trainer_clips_and_repeats_bit_for_bit_in_deterministic_mode(dev):
    from test_deterministic_mode_gpu import _lora_model

    from clibd_amd.data import synthetic_batch
    from clibd_amd.train import Trainer

    batch = synthetic_batch(8, dev, seed=3, rank=0, with_text=False)
    runs = []
    for _ in range(2):
        model = _lora_model(dev, text=False)
        model.train(True)
        tr = Trainer(model, lr=1e-4, world_size=1, rank=0, all_gather=True, deterministic=True, max_grad_norm=1.0)
        assert tr.optimizer.max_grad_norm == 1.0 and tr.optimizer.nonfinite == "propagate" and len(tr.optimizer.param_groups) == 1
        torch.manual_seed(123)
        before = tr.optimizer.flat_p.clone()
        tr.step(batch["image"], batch["dna"], batch["text"], batch["labels"])
        torch.cuda.synchronize()
        runs.append((tr.optimizer.flat_p.clone(), tr.optimizer.grad_norm.item(), tr.optimizer._record.view(F32)[1].item()))
        assert not torch.equal(before, runs[-1][0])
    print("Trainer: grad_norm", runs[0][1], runs[1][1], "coef", runs[0][2])
    assert np.isfinite(runs[0][1]) and runs[0][1] > 0 and runs[0][1] == runs[1][1] and 0 < runs[0][2] <= 1.0
    assert torch.equal(runs[0][0], runs[1][0])


# ---- 7. checkpoint ------------------------------------------------------------------------------------------------------------------------------
def test_training_state_round_trips_two_groups(dev, tmp_path):
    from clibd_amd.checkpoint import load_training_state, save_training_state
    from clibd_amd.optim import FusedAdamW, decay_parameter_groups

    def make(seed, lrs, wd):
        torch.manual_seed(seed)
        model = torch.nn.Sequential(torch.nn.Linear(24, 10), torch.nn.LayerNorm(10), torch.nn.Linear(10, 3)).to(dev)
        groups = decay_parameter_groups(model, wd)
        for g, lr in zip(groups, lrs):
            g["lr"] = lr
        return model, FusedAdamW(groups, max_grad_norm=1.0)

    model, opt = make(1, (1e-3, 5e-3), 0.05)
    assert [len(g["params"]) for g in opt.param_groups] == [2, 4] and opt._group_first == [0, 320]
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        _feed(opt, [torch.randn(p.shape, generator=gen) for p in opt.bucket_params()])
        opt.step()
    path = str(tmp_path / "state.pth")
    save_training_state(path, model, opt, epoch=3)
    saved = torch.load(path, weights_only=False)["optimizer"]
    assert [e[0] for e in saved["layout"]] == ["0.weight", "2.weight", "0.bias", "1.weight", "1.bias", "2.bias"]
    assert [e[1] for e in saved["layout"]] == opt._offsets and len(saved["param_groups"]) == 2
    model2, opt2 = make(2, (7e-2, 7e-2), 0.9)
    assert load_training_state(path, model2, opt2) == 3
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and torch.equal(opt2.flat_p, opt.flat_p)
    assert opt2.step_count == 2 and bool((opt2.exp_avg != 0).any())
    assert [(g["lr"], g["weight_decay"]) for g in opt2.param_groups] == [(1e-3, 0.05), (5e-3, 0.0)]
    torch.manual_seed(1)
    model1 = torch.nn.Sequential(torch.nn.Linear(24, 10), torch.nn.LayerNorm(10), torch.nn.Linear(10, 3)).to(dev)
    with pytest.raises(ValueError, match="parameter groups"):                  # a one-group optimizer cannot take two groups' hyperparameters
        load_training_state(path, model1, FusedAdamW(model1.parameters()))
    save_training_state(path, model1, FusedAdamW(model1.parameters(), lr=3e-3), epoch=1)      # a one-group file loads as before
    one = FusedAdamW(model1.parameters(), lr=9.0)
    assert load_training_state(path, model1, one) == 1 and one.param_groups[0]["lr"] == 3e-3
