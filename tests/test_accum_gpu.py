"""GPU checks of gradient accumulation and data-parallel masked-LM pre-training (clibd_amd.optim, clibd_amd.mlm, include/clibd_hip_accum.h).

Kernel: clibd_grad_norm_div against clibd_grad_norm bit for bit where the divisor is NULL, 1 or 0, and against the fp64 restatement of
tests/accum_reference.py at the gate of tests/test_optim_gpu.py::test_norm_against_fp64 (3 x the error of the fp32 restatement in the
kernel's order against fp64, floor 2^-22).  Optimizer: a window of k micro-steps bit for bit against a k = 1 optimizer stepping once on the
same bucket content with grad_scale / k.  The invariant: one batch of 8 sequences, 4 micro-batches of 2, and 2 ranks x 2 micro-batches
each meet the gates of tests/test_mlm_gpu.py against the CPU oracle's big-batch loss and gradient (loss 1e-3; rel 3e-2, cosine 0.999), with
label counts per micro-batch (9, 0, 1, 5) for which the mean of micro-batch means misses those gates.  Every figure is printed before it is
asserted.

Measured on an MI355X: see DESIGN §3.18."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import accum_reference as AR  # noqa: E402
import mlm_labels_reference as LR  # noqa: E402
import mlm_reference as MR  # noqa: E402
import optim_reference as OR  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------------
def run_norm(ops, g, divisor="none", grad_scale=1.0, max_norm=None, skip=False, record=None):
    """clibd_grad_norm (divisor="none") or clibd_grad_norm_div with the workspace inside a poisoned buffer: (record on the CPU, its float
    view, workspace tail intact)"""
    dev = g.device
    if record is None:
        record = torch.zeros((4,), dtype=torch.int32, device=dev)
    need = ops.grad_norm_workspace(g.numel(), dev).numel()
    buf = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=dev)
    if isinstance(divisor, str):
        ops.grad_norm(g, record, buf[:need], grad_scale, max_norm, skip)
    else:
        d = None if divisor is None else torch.tensor([divisor], dtype=F32, device=dev)
        ops.grad_norm_div(g, record, buf[:need], d, grad_scale, max_norm, skip)
    rec = record.cpu()
    chunks = max(1, -(-g.numel() // OR.CHUNK))
    return rec, rec.view(F32), bool((buf[4 * chunks:] == 0xAB).all())


@pytest.mark.parametrize("divisor", AR.DIVISORS)
@pytest.mark.parametrize("n", AR.SIZES)
def test_norm_div_against_grad_norm_and_fp64(dev, n, divisor):
    from clibd_amd import ops

    gs = 0.25
    g_np = OR.gradient(n)
    g = torch.from_numpy(g_np).to(dev)
    ref, gate, err32 = AR.norm_div_gate(g_np, gs, divisor)
    for max_norm in (0.5 * ref, None, 4.0 * ref + 1e-5):
        rec, recf, intact = run_norm(ops, g, divisor, gs, max_norm, skip=True)
        got, coef = float(recf[0]), recf[1].item()
        assert intact and rec[2].item() == 0 and rec[3].item() == 0
        if float(AR.divisor_of(divisor)) == 1.0:                # NULL, 1 and 0: clibd_grad_norm's record, bit for bit
            base, _, _ = run_norm(ops, g, "none", gs, max_norm, skip=True)
            assert torch.equal(rec, base), (n, divisor, max_norm, rec.tolist(), base.tolist())
        err = abs(got - ref) / ref
        print(f"norm_div n={n} divisor={divisor} max_norm={max_norm}: kernel {got:.9g}, fp64 {ref:.9g}, rel err {err:.3e}, fp32 restatement {err32:.3e}, "
              f"gate {gate:.3e}, coef {coef:.9g}")
        assert err <= gate
        assert coef == float(AR.coef_div(np.float32(got), max_norm, divisor))   # torch's formula on the kernel's own norm, then / d, in fp32
        if max_norm is not None and max_norm < ref:
            assert 0 < coef * float(AR.divisor_of(divisor)) < 1
    rec2, _, _ = run_norm(ops, g, divisor, gs, 0.5 * ref, skip=True)          # two runs are bit-equal
    rec3, _, _ = run_norm(ops, g, divisor, gs, 0.5 * ref, skip=True)
    assert torch.equal(rec2, rec3)


def test_norm_div_nonfinite_values_set_skip_now(dev):
    from clibd_amd import ops

    n = 3 * OR.CHUNK + 5
    for bad, where in ((float("inf"), 0), (float("-inf"), n - 1), (float("nan"), OR.CHUNK + 17)):
        g = torch.from_numpy(OR.gradient(n)).to(dev)
        g[where] = bad
        record = torch.zeros((4,), dtype=torch.int32, device=dev)
        rec, recf, _ = run_norm(ops, g, 7.0, 1.0, max_norm=1.0, skip=True, record=record)
        print(f"{bad} at {where}, divisor 7, skip on:", recf[:2].tolist(), rec[2:].tolist())
        assert not np.isfinite(recf[0].item()) and (np.isnan(recf[0].item()) == np.isnan(bad)) and rec[2:].tolist() == [1, 1]
        rec, _, _ = run_norm(ops, g, 7.0, 1.0, max_norm=1.0, skip=True, record=record)       # the count accumulates
        assert rec[2:].tolist() == [1, 2]
        rec, recf, _ = run_norm(ops, g, 7.0, 1.0, max_norm=1.0, skip=False, record=record)   # skip off: non-finite norm, no flag
        assert not np.isfinite(recf[0].item()) and rec[2:].tolist() == [0, 2]
        g[where] = 1.0
        rec, recf, _ = run_norm(ops, g, 7.0, 1.0, max_norm=1.0, skip=True, record=record)    # a clean gradient clears skip_now
        assert np.isfinite(recf[0].item()) and rec[2:].tolist() == [0, 2]


# ---- 2. the optimizer's window ----------------------------------------------------------------------------------------------------------------
SHAPES = [[(5, 64), (100,)], [(), (70,), (1000,)]]      # two groups: starts 0 and 448; a bucket of 1664 floats


def _optimizers(dev, kind, k, groups, **kw):
    """(windowed optimizer, k = 1 optimizer) over equal parameters, each with its own copy"""
    from clibd_amd.optim import FusedAdam, FusedAdamW

    cls = FusedAdamW if kind == "adamw" else FusedAdam
    gen = torch.Generator().manual_seed(21)
    vals = [[torch.randn(s, generator=gen) * 0.1 for s in grp] for grp in SHAPES]
    out = []
    for steps in (k, 1):
        ps = [[torch.nn.Parameter(v.clone().to(dev)) for v in grp] for grp in vals]
        if groups:
            arg = [{"params": ps[0], "lr": 1e-3, "weight_decay": 0.1}, {"params": ps[1], "lr": 5e-3, "weight_decay": 0.0}]
        else:
            arg = ps[0] + ps[1]
        out.append(cls(arg, lr=2e-3, weight_decay=0.05, accumulation_steps=steps, **kw))
    return out


def _state(opt):
    return [t.clone() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq)]


def _same(opt, state):
    return all(torch.equal(a, b) for a, b in zip(_state(opt), state))


@pytest.mark.parametrize("mode", ["plain", "groups_clip", "flush", "skip"])
@pytest.mark.parametrize("kind", ["adamw", "adam_l2"])
def test_window_equals_one_step_on_the_same_bucket(dev, kind, mode):
    kw = {"plain": {}, "flush": {}, "groups_clip": dict(max_grad_norm=0.05), "skip": dict(max_grad_norm=1.0, nonfinite="skip")}[mode]
    win, ref = _optimizers(dev, kind, 3, mode in ("groups_clip", "skip"), **kw)
    win.grad_scale = ref_scale = 0.5
    n = win.flat_g.numel()
    gen = torch.Generator().manual_seed(22)
    for window in range(2):
        taken = 2 if mode == "flush" else 3
        for micro in range(taken):
            before = _state(win)
            win.zero_grad()
            g = torch.randn(n, generator=gen).to(dev)
            if mode == "skip" and window == 0 and micro == 1:
                g[777] = float("inf")
            win.flat_g.add_(g)                                   # the gradient written straight into the bucket
            win.aux[7] += 1.0
            win.step()
            if micro < taken - 1 or mode == "flush":
                assert _same(win, before) and win.step_count == window and win.window_open   # calls 1 and 2: p, m and v keep their bits
        if mode == "flush":
            assert win.flush() is True
        assert not win.window_open and win.step_count == window + 1 and float(win.aux[7]) == taken
        ref.zero_grad()
        ref.flat_g.copy_(win.flat_g)                             # the same bucket content
        ref.grad_scale = ref_scale / taken
        before_ref = _state(ref)
        ref.step()
        diffs = [int((a != b).sum()) for a, b in zip(_state(win), _state(ref))]
        print(f"{kind} {mode} window {window}: elements that differ from the k = 1 step (p, m, v): {diffs}; norm {float(win.grad_norm):.6g}, "
              f"skipped {int(win.skipped_steps)}")
        assert diffs == [0, 0, 0] and torch.equal(win._record, ref._record)
        if mode == "skip" and window == 0:
            assert _same(win, before) and _same(ref, before_ref) and int(win.skipped_steps) == 1     # a skipped window: nothing moved
        else:
            assert not torch.equal(win.flat_p, before[0])
        if mode == "groups_clip":
            assert 0 < float(win._record.view(F32)[1]) < 1       # the clip was active on the averaged gradient
    assert int(win.skipped_steps) == (1 if mode == "skip" else 0)


@pytest.mark.parametrize("kind", ["adamw", "adam_l2"])
def test_device_divisor_window_equals_one_step_with_that_scale(dev, kind):
    """divisor_slot: aux[4] = 3 + 4 = 7 summed on the device over two micro-steps; the update equals a k = 1 plain step with grad_scale 1/7
    (fp32(1) * fp32(1 / 7) is what a float 1/7 argument rounds to)"""
    win, ref = _optimizers(dev, kind, 2, False)
    win.divisor_slot = 4
    gen = torch.Generator().manual_seed(23)
    for count in (3.0, 4.0):
        win.zero_grad()
        win.flat_g.add_(torch.randn(win.flat_g.numel(), generator=gen).to(dev))
        win.aux[4] += count
        win.step()
    assert win.step_count == 1 and float(win.aux[4]) == 7.0
    ref.zero_grad()
    ref.flat_g.copy_(win.flat_g)
    ref.grad_scale = 1.0 / 7.0
    ref.step()
    diffs = [int((a != b).sum()) for a, b in zip(_state(win), _state(ref))]
    print(f"{kind} device divisor 7: elements that differ from the k = 1 step with grad_scale 1/7 (p, m, v): {diffs}; record {win._record.view(F32)[:2].tolist()}")
    assert diffs == [0, 0, 0]


# ---- 3. the invariant: one big batch = k micro-batches = W ranks x k micro-batches --------------------------------------------------------------
CFG = dict(vocab_size=259, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, max_position_embeddings=136)
NO_DROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
S, B = 17, 8
COUNTS = (9, 0, 1, 5)            # labelled positions of the micro-batches (sequences 2i, 2i + 1): unequal, one empty
PORT = 29671


def invariant_case():
    """(ids, labels) int64 [8, 17], fixed: the labels sit at hashed positions, COUNTS[i] of them in micro-batch i"""
    g = torch.Generator().manual_seed(1808)
    ids = torch.cat([torch.ones(B, 1, dtype=torch.long), torch.randint(3, CFG["vocab_size"], (B, S - 1), generator=g)], dim=1)
    labels = torch.full((B, S), -100, dtype=torch.long)
    for i, c in enumerate(COUNTS):
        where = torch.randperm(2 * S, generator=g)[:c]
        for w in where.tolist():
            b, s = 2 * i + w // S, w % S
            labels[b, s] = ids[b, s]
            ids[b, s] = 0                # <MASK>
    assert [int((labels[2 * i:2 * i + 2] != -100).sum()) for i in range(4)] == list(COUNTS)
    return ids, labels


def _shapes():
    from clibd_amd.model import BertConfigLite, BertForMaskedLM

    return {k: tuple(v.shape) for k, v in BertForMaskedLM(BertConfigLite(**CFG)).state_dict().items()}


def _state_dict(tied):
    sd = MR.synth_state(1809, _shapes())
    if tied:
        sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
        sd["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"]
    return sd


def _model(tied, dev, k=1, perturb=0.0):
    from clibd_amd import mlm
    from clibd_amd.model import BertConfigLite, BertForMaskedLM
    from clibd_amd.optim import FusedAdamW

    m = mlm.BarcodeBERTForPreTraining(BertForMaskedLM(BertConfigLite(**CFG, **NO_DROP)), tie_word_embeddings=tied)
    m.load_state_dict(_state_dict(tied), strict=True)
    m = m.to(dev).train()
    if perturb:
        with torch.no_grad():
            for p in m.parameters():
                p.add_(perturb)
    opt = FusedAdamW(m.parameters(), lr=1e-3, accumulation_steps=k)
    m.attach(opt)
    return m, opt


def _grads(model, divisor=1.0):
    """{HF key: gradient in the optimizer's bucket / divisor (CPU)}; a tied parameter under both names"""
    return {n: (p.grad.detach() / divisor).cpu() for n, p in model.named_parameters(remove_duplicate=False)}


_oracle = {}


def oracle(tied):
    """the CPU oracle's big-batch loss and gradients (bf16 rounding points), and its mean of the four micro-batch means: computed once"""
    if tied not in _oracle:
        from oracle import clibd_oracle as O

        ids, labels = invariant_case()
        ones = torch.ones_like(ids)
        om = MR.oracle_for(CFG, _state_dict(tied), tied)
        with O.precision("bf16"):
            lo, _ = LR.labels_loss(om, ids, ones, labels)
            go = MR.named_grads(om, lo)
        _oracle[tied] = (float(lo.detach()), go)
    return _oracle[tied]


def distances(got, ref):
    """(worst relative distance, worst cosine) over the tensors assert_grads compares by those two"""
    from test_model_gpu import cos, rel

    gmax = max(float(r.abs().max()) for r in ref.values())
    keys = [n for n in ref if ref[n].abs().max() >= max(2e-6, 1e-4 * gmax)]
    return max(float(rel(got[n], ref[n])) for n in keys), min(float(cos(got[n], ref[n])) for n in keys)


def gate(got, loss, tied, what):
    """the gates of tests/test_mlm_gpu.py::test_loss_and_gradients_match_golden_and_oracle against the oracle, number for number"""
    from test_model_gpu import assert_grads

    lo, go = oracle(tied)
    worst_rel, worst_cos = distances(got, go)
    print(f"{what} tied={tied}: loss {loss:.6f} (oracle {lo:.6f}, off by {abs(loss - lo):.2e}); gradients: worst rel {worst_rel:.4e}, worst cosine {worst_cos:.6f}")
    assert abs(loss - lo) < 1e-3
    assert_grads(got, go, rel_tol=3e-2, cos_tol=0.999, what=f"{what} tied={tied} vs oracle-bf16", zero_tol=2e-6, zero_rel=1e-4)
    return worst_rel, worst_cos


def _rank_worker(rank, world, port, out, ndev, tied):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist

    torch.cuda.set_device(rank % ndev)
    dev = torch.device("cuda", rank % ndev)
    if ndev >= world:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)   # ranks share a GPU: device tensors travel through gloo
    try:
        from clibd_amd import mlm

        ids, labels = invariant_case()
        m, opt = _model(tied, dev, k=2, perturb=0.01 * rank)          # rank 1 starts elsewhere: the epoch must broadcast rank 0's values
        sl = slice(4 * rank, 4 * rank + 4)                           # the caller shards: rank r takes micro-batches 2r and 2r + 1
        loader = [{"input_ids": ids[sl][j:j + 2], "labels": labels[sl][j:j + 2]} for j in (0, 2)]
        calls = []
        real = dist.all_reduce
        dist.all_reduce = lambda t, *a, **k: (calls.append(t.numel()), real(t, *a, **k))[1]
        stats = mlm.pretrain_epoch(m, loader, opt, accumulation_steps=2, world_size=world, rank=rank)
        dist.all_reduce = real
        torch.cuda.synchronize()
        count = float(opt.aux[mlm.AUX_COUNT])
        res = {"stats": stats, "count": count, "loss": float(opt.aux[mlm.AUX_LOSS]) / count, "grads": _grads(m, count), "collectives": calls,
               "bucket": opt.flat_comm.numel(), "grad_scale": opt.grad_scale, "step_count": opt.step_count, "p": opt.flat_p.cpu()}
        # identical ids on both ranks: the masks must differ (the seed is the same CPU draw on both; rank and micro-step enter the hash)
        torch.manual_seed(5)
        same = ids[:2].to(dev)
        a = mlm.pretrain_step(m, same, opt, 0.5, accumulation_steps=2, world_size=world, rank=rank)
        b = mlm.pretrain_step(m, same, opt, 0.5, accumulation_steps=2, world_size=world, rank=rank)
        torch.cuda.synchronize()
        res.update(mask_losses=[float(a[0]), float(b[0])], p2=opt.flat_p.cpu(), step_count2=opt.step_count)
        # evaluate: each rank scores its shard; one all-reduce of the three sums makes every rank return the global figures
        shard = [ids[sl][:3], ids[sl][3:]]
        res.update(eval_local=mlm.evaluate(m, shard, seed=2, rank=rank), eval_global=mlm.evaluate(m, shard, seed=2, world_size=world, rank=rank),
                   p3=opt.flat_p.cpu())
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("tied", [True, False])
def test_big_batch_equals_micro_batches_equals_ranks_times_micro_batches(dev, tied):
    from clibd_amd import mlm

    ids, labels = invariant_case()
    # (a) one batch of 8 sequences, the step as it always was
    ma, oa = _model(tied, dev)
    la, _, na = mlm.pretrain_step(ma, ids.to(dev), oa, labels=labels.to(dev))
    assert int(na) == sum(COUNTS) and oa.divisor_slot is None
    da = gate(_grads(ma), float(la), tied, "(a) one batch of 8")
    # (b) k = 4 micro-batches of 2
    mb, ob = _model(tied, dev, k=4)
    start = ob.flat_p.clone()
    for i in range(4):
        assert ob.window_closes == (i == 3)
        mlm.pretrain_step(mb, {"input_ids": ids[2 * i:2 * i + 2].to(dev), "labels": labels[2 * i:2 * i + 2].to(dev)}, ob, accumulation_steps=4)
        assert torch.equal(ob.flat_p, start) == (i < 3)
    count = float(ob.aux[mlm.AUX_COUNT])
    assert count == sum(COUNTS) and ob.step_count == 1 and ob.divisor_slot == mlm.AUX_COUNT
    db = gate(_grads(mb, count), float(ob.aux[mlm.AUX_LOSS]) / count, tied, "(b) 4 micro-batches of 2")
    upd = ((ob.flat_p - oa.flat_p).double().norm() / (oa.flat_p - start).double().norm()).item()
    print(f"(b) vs (a) tied={tied}: distance of the parameter updates relative to the update's norm {upd:.3e}")
    # the mean of the micro-batch means is another gradient: it misses the gates (a) and (b) meet
    mm, om_ = _model(tied, dev, k=4)
    means = []
    for i in range(4):
        om_.zero_grad()
        loss, _ = mm(input_ids=ids[2 * i:2 * i + 2].to(dev), labels=labels[2 * i:2 * i + 2].to(dev))
        loss.backward()
        om_.step()
        means.append(float(loss.detach()))
    assert om_.step_count == 1
    dm = distances(_grads(mm, 4.0), oracle(tied)[1])
    print(f"mean of means tied={tied}: loss {sum(means) / 4:.6f} (oracle big batch {oracle(tied)[0]:.6f}); gradients: worst rel {dm[0]:.4e}, worst cosine {dm[1]:.6f}")
    assert dm[0] > 3e-2 and abs(sum(means) / 4 - oracle(tied)[0]) > 1e-3
    # (c) W = 2 ranks x k = 2 micro-batches: two processes (sharing the GPU over gloo on a 1-GPU box)
    import torch.multiprocessing as mp

    n = torch.cuda.device_count()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_rank_worker, args=(2, PORT + int(tied), out, n, tied), nprocs=2, join=True)
    res = dict(out)
    assert sorted(res) == [0, 1]
    for r in (0, 1):
        x = res[r]
        dc = gate(x["grads"], x["loss"], tied, f"(c) rank {r} of 2 x 2 micro-batches")
        assert x["count"] == sum(COUNTS) and x["step_count"] == 1 and x["grad_scale"] == 1.0
        assert x["collectives"] == [x["bucket"]]                         # ONE all-reduce per window: the flat bucket with its aux slots
        assert x["stats"]["steps"] == 1 and abs(x["stats"]["loss"] - x["loss"]) < 1e-6 and x["stats"]["skipped"] == 0
        assert x["step_count2"] == 2
    assert torch.equal(res[0]["p"], res[1]["p"]) and torch.equal(res[0]["p2"], res[1]["p2"])       # both ranks end with the same parameters
    assert not torch.equal(res[0]["p"], res[0]["p2"])
    assert len({round(v, 4) for r in (0, 1) for v in res[r]["mask_losses"]}) == 4                  # identical ids: four different masks
    loc, glo = [res[r]["eval_local"] for r in (0, 1)], [res[r]["eval_global"] for r in (0, 1)]
    tokens = loc[0]["tokens"] + loc[1]["tokens"]
    want = (loc[0]["loss"] * loc[0]["tokens"] + loc[1]["loss"] * loc[1]["tokens"]) / tokens
    print(f"evaluate over 2 ranks tied={tied}: global {glo[0]}, shards {loc}")
    assert glo[0] == glo[1] and glo[0]["tokens"] == tokens and loc[0] != loc[1] and abs(glo[0]["loss"] - want) <= 1e-12 * want
    assert abs(glo[0]["accuracy"] - (loc[0]["accuracy"] * loc[0]["tokens"] + loc[1]["accuracy"] * loc[1]["tokens"]) / tokens) <= 1e-12
    assert all(torch.equal(res[r]["p3"], res[r]["p2"]) for r in (0, 1))
    updc = ((res[0]["p"].to(dev) - oa.flat_p).double().norm() / (oa.flat_p - start).double().norm()).item()
    print(f"(c) vs (a) tied={tied}: distance of the parameter updates relative to the update's norm {updc:.3e}")
    print(f"DISTANCES tied={tied}: (a) rel {da[0]:.4e} cos {da[1]:.6f}; (b) rel {db[0]:.4e} cos {db[1]:.6f}; (c) rel {dc[0]:.4e} cos {dc[1]:.6f}")


def test_ranks_and_micro_steps_draw_different_masks(dev):
    from clibd_amd import mlm

    ids = invariant_case()[0].to(dev)
    drawn = [mlm.mask_tokens(ids, 0.5, mlm.micro_seed(5, r, m))[0] for r in (0, 1) for m in (0, 1)]
    assert all(not torch.equal(a, b) for i, a in enumerate(drawn) for b in drawn[i + 1:])
    assert torch.equal(drawn[0], mlm.mask_tokens(ids, 0.5, mlm.micro_seed(5, 0, 0))[0])


def test_epoch_with_k_1_equals_the_plain_loop_bit_for_bit(dev):
    """k = 1, W = 1, dropout on: pretrain_epoch and the plain loop of pretrain_step draw the same seeds and launch the same kernels"""
    from clibd_amd import mlm
    from clibd_amd.model import BertConfigLite, BertForMaskedLM
    from clibd_amd.optim import FusedAdamW

    g = torch.Generator().manual_seed(31)
    batches = [torch.cat([torch.ones(b, 1, dtype=torch.long), torch.randint(3, 259, (b, S - 1), generator=g)], dim=1) for b in (3, 2, 4)]

    def build():
        m = mlm.BarcodeBERTForPreTraining(BertForMaskedLM(BertConfigLite(**CFG)), tie_word_embeddings=True)
        m.load_state_dict(_state_dict(True), strict=True)
        m = m.to(dev).set_deterministic(True)
        return m, FusedAdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0)

    m1, o1 = build()
    torch.manual_seed(32)
    stats = mlm.pretrain_epoch(m1, batches, o1, sampler="bert", mlm_probability=0.3)
    m2, o2 = build()
    m2.attach(o2)
    m2.train()
    torch.manual_seed(32)
    tot = torch.zeros(3, dtype=torch.float64)
    for b in batches:
        loss, correct, n_valid = mlm.pretrain_step(m2, b, o2, sampler="bert", mlm_probability=0.3)
        tot += torch.tensor([float(loss), float(correct), float(n_valid)], dtype=torch.float64)
    assert torch.equal(o1.flat_p, o2.flat_p) and torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    assert o1.step_count == o2.step_count == 3 and o1.divisor_slot is None and o1.accumulation_steps == 1
    assert stats["steps"] == 3 and stats["skipped"] == 0 and sorted(stats) == ["accuracy", "loss", "skipped", "steps"]
    assert abs(stats["loss"] - float(tot[0]) / 3) < 1e-12 and abs(stats["accuracy"] - float(tot[1]) / float(tot[2])) < 1e-12


def test_epoch_windows_flush_and_scheduler(dev):
    """5 micro-batches with k = 2: two full windows and a flushed one; the scheduler steps once per update"""
    from clibd_amd import mlm

    m, opt = _model(True, dev, k=2)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    g = torch.Generator().manual_seed(33)
    batches = [torch.cat([torch.ones(2, 1, dtype=torch.long), torch.randint(3, 259, (2, S - 1), generator=g)], dim=1) for _ in range(5)]
    stats = mlm.pretrain_epoch(m, batches, opt, sched, seed=9)
    print("k = 2 over 5 micro-batches:", stats)
    assert stats["steps"] == 3 and opt.step_count == 3 and not opt.window_open
    assert abs(opt.param_groups[0]["lr"] - 1e-3 * 0.5 ** 3) < 1e-12
    assert 0 < stats["loss"] < 20 and 0 <= stats["accuracy"] <= 1


# ---- 4. evaluate ------------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_is_the_token_weighted_mean_and_touches_nothing(dev):
    """Against model(...) batch by batch on the same masks.  Both sides divide the same fp32 sum of row losses — by 1 here, by n_valid there,
    one rounding of 2^-24 relative — so the token-weighted totals agree within 2^-22 relative; hits and counts are integers."""
    from clibd_amd import mlm

    m, opt = _model(False, dev)
    opt.exp_avg.add_(0.25)
    m.train()
    g = torch.Generator().manual_seed(41)
    batches = [torch.cat([torch.ones(b, 1, dtype=torch.long), torch.randint(3, 259, (b, S - 1), generator=g)], dim=1) for b in (4, 1, 3)]
    batches[1][0, 5:] = 2                     # mostly padding k-mers: fewer valid targets
    before = [t.clone() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.flat_comm)]
    res = mlm.evaluate(m, batches, seed=3)
    assert m.training and opt.step_count == 0 and all(torch.equal(a, b) for a, b in zip(before, (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.flat_comm)))
    m.eval()
    tot_loss, hits, tokens = 0.0, 0, 0
    with torch.no_grad():
        for i, b in enumerate(batches):
            masked, rows, targets, n_valid = mlm.mask_tokens(b.to(dev), 0.5, mlm.micro_seed(3, 0, i))
            loss, correct = m(masked, rows, targets, n_valid)
            tot_loss += float(loss.double()) * int(n_valid)
            hits += int(correct)
            tokens += int(n_valid)
    want = tot_loss / tokens
    print(f"evaluate: loss {res['loss']:.9f} (batch by batch {want:.9f}, rel {abs(res['loss'] - want) / want:.2e}), accuracy {res['accuracy']:.6f}, "
          f"perplexity {res['perplexity']:.4f}, tokens {res['tokens']}")
    assert sorted(res) == ["accuracy", "loss", "perplexity", "tokens"]
    assert res["tokens"] == tokens and tokens < sum(b.shape[0] for b in batches) * 8 and res["accuracy"] == hits / tokens
    assert abs(res["loss"] - want) <= 2.0 ** -22 * want
    assert abs(res["perplexity"] - float(np.exp(res["loss"]))) < 1e-9 * res["perplexity"]
    assert mlm.evaluate(m, batches, seed=3) == res and mlm.evaluate(m, batches, seed=4) != res      # the seed fixes the masks
    assert not m.training
