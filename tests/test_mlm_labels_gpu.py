"""GPU checks of the masked-LM labels (clibd_amd.mlm's HF-style call, include/clibd_hip_mlm_labels.h).

Compaction, sampler, gather and scatter with padding rows: exact against tests/mlm_labels_reference.py / torch indexing, with guard
elements on both sides of every output.
Equivalence: the HF-style call fed the fixed-count sampler's rows equals the existing call bit for bit; with 64 padding rows more the
gradient of the top hidden state is still bit-equal.
End to end against tests/golden/mlm_labels_golden.pt (HF fp32, attention mask, free labels) and the oracle in bf16 mode at exactly the
gates of tests/test_mlm_gpu.py::test_loss_and_gradients_match_golden_and_oracle (restated below with that test's numbers: oracle loss
1e-3, gradients rel 3e-2, cosine 0.999, zero_tol 2e-6, zero_rel 1e-4; HF loss rel 2e-2, gradients rel 5e-2, cosine 0.998, norms 5e-2).
The masked cases run the masked attention kernels, which tests/test_attention_forms_gpu.py holds to fp64.

Measured on an MI355X: see DESIGN §3.16."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import mlm_labels_reference as LR  # noqa: E402
import mlm_reference as MR  # noqa: E402
from test_mlm_gpu import grads_by_key, pretraining_model, tied_state  # noqa: E402  (the builders of the existing path's tests)
from test_model_gpu import assert_grads  # noqa: E402  (the gates' own code)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
A = LR.A
WIDE = dict(vocab_size=1027, hidden_size=256, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
SHAPES = [(1, 2), (3, 17), (5, 133), (64, 256), (512, 256)]


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "mlm_labels_golden.pt", weights_only=False)


def pad64(n):
    return (n + 63) // 64 * 64


# ---- 1. compaction ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64
ROW_POISON, TGT_POISON = -777, -(1 << 40)


def run_compact(labels, V, r_cap, dev):
    """the C entry on outputs that sit inside poisoned buffers: (rows, targets, n, overflow word, guards intact)"""
    from clibd_amd import _lib, ops

    L = _lib.load()
    M = labels.numel()
    rows = torch.full((r_cap + 2 * GUARD,), ROW_POISON, dtype=torch.int32, device=dev)
    targets = torch.full((r_cap + 2 * GUARD,), TGT_POISON, dtype=torch.int64, device=dev)
    small = torch.full((8,), ROW_POISON, dtype=torch.int32, device=dev)          # n at [2], the overflow word at [5]
    small[5] = 0
    ws = torch.empty((L.clibd_mlm_compact_workspace_bytes(M),), dtype=torch.uint8, device=dev)
    lab = labels.to(dev)
    _lib.check(L.clibd_mlm_compact_labels(lab.data_ptr(), M, V, r_cap, rows[GUARD:].data_ptr(), targets[GUARD:].data_ptr(), small[2:].data_ptr(),
                                          small[5:].data_ptr(), ops.ce_error_word(dev).data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
               "mlm_compact_labels")
    rows, targets, small = rows.cpu(), targets.cpu(), small.cpu()
    intact = bool((rows[:GUARD] == ROW_POISON).all() and (rows[GUARD + r_cap:] == ROW_POISON).all() and (targets[:GUARD] == TGT_POISON).all()
                  and (targets[GUARD + r_cap:] == TGT_POISON).all() and (small[[0, 1, 3, 4, 6, 7]] == ROW_POISON).all())
    return rows[GUARD:GUARD + r_cap].numpy(), targets[GUARD:GUARD + r_cap].numpy(), int(small[2]), int(small[5]), intact


def label_patterns(M, V):
    g = torch.Generator().manual_seed(M)
    vals = torch.randint(0, V, (M,), generator=g)
    none = torch.full((M,), LR.IGNORE, dtype=torch.int64)
    out = {"none": none, "all": vals.clone()}
    first, last = none.clone(), none.clone()
    first[0], last[M - 1] = vals[0], vals[M - 1]
    out["first"], out["last"] = first, last
    for name, p in (("p15", 0.15), ("p50", 0.5)):
        out[name] = torch.where(torch.rand(M, generator=g) < p, vals, none)
    if M >= 192:                                             # a count that is a multiple of 64: the capacity can equal it
        n = max(64, M // 3 // 64 * 64)
        exact = none.clone()
        idx = torch.randperm(M, generator=g)[:n]
        exact[idx] = vals[idx]
        out["exact"] = exact
    return out


@pytest.mark.parametrize("B,S", SHAPES)
def test_compaction_equals_numpy(dev, B, S):
    from clibd_amd import ops

    M, V = B * S, 259
    ops.ce_error_word(dev).zero_()
    for name, labels in label_patterns(M, V).items():
        n = int((labels != LR.IGNORE).sum())
        caps = {pad64(M), min(pad64(M), max(64, pad64(n))), min(pad64(M), pad64(n) + 64)}
        if name == "exact":
            assert n % 64 == 0 and {n, n + 64} <= caps          # the capacity exactly the count, and the count + 64
        if pad64(n) - 64 >= 64 and pad64(n) - 64 < n:
            caps.add(pad64(n) - 64)                              # one granule too small
        for r_cap in sorted(caps):
            want_rows, want_targets, want_n, want_over = LR.compact(labels.numpy(), r_cap)
            rows, targets, got_n, over, intact = run_compact(labels, V, r_cap, dev)
            assert intact, (name, r_cap)
            assert got_n == want_n == n and over == int(want_over) == int(n > r_cap), (name, r_cap, got_n, over)
            assert np.array_equal(rows, want_rows) and np.array_equal(targets, want_targets), (name, r_cap)
        if name in ("p15", "exact"):                               # the wrapper, default capacity, and a second launch: the same bits
            r1, t1, n1 = ops.mlm_compact_labels(labels.to(dev).view(B, S), V)
            r2, t2, n2 = ops.mlm_compact_labels(labels.to(dev).view(B, S), V)
            w = LR.compact(labels.numpy(), pad64(M))
            assert r1.dtype == torch.int32 and t1.dtype == torch.int64 and n1.dtype == torch.int32 and r1.numel() == pad64(M)
            assert np.array_equal(r1.cpu().numpy(), w[0]) and np.array_equal(t1.cpu().numpy(), w[1]) and int(n1) == w[2]
            assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(n1, n2)
    assert int(ops.ce_error_word(dev)) == 0 and int(ops.mlm_overflow_word(dev)) == 0
    if M >= 17:                                                    # a label outside [0, V) that is not -100: the cross-entropy's error word
        bad = label_patterns(M, V)["p15"]
        bad[M // 2] = V
        rows, targets, got_n, over, intact = run_compact(bad, V, pad64(M), dev)
        assert intact and int(ops.ce_error_word(dev)) & 1 and M // 2 in rows.tolist()          # flagged, and passed through
        ops.ce_error_word(dev).zero_()
        bad[M // 2] = -1
        run_compact(bad, V, pad64(M), dev)
        assert int(ops.ce_error_word(dev)) & 1
        ops.ce_error_word(dev).zero_()


def test_overflow_word_is_sticky(dev):
    from clibd_amd import ops

    labels = torch.arange(300, dtype=torch.int64, device=dev) % 7
    word = torch.zeros((1,), dtype=torch.int32, device=dev)
    rows, targets, n = ops.mlm_compact_labels(labels, 259, 128, overflow=word)
    assert int(word) == 1 and int(n) == 300 and rows.tolist() == list(range(128))
    ops.mlm_compact_labels(labels[:64].contiguous(), 259, 64, overflow=word)          # fits: the word stays set
    assert int(word) == 1
    with pytest.raises(ValueError):
        ops.mlm_compact_labels(labels, 259, 100)
    with pytest.raises(ValueError):
        ops.mlm_compact_labels(labels, 259, 384)


# ---- 2. the sampler --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(1, 2), (3, 17), (5, 133), (4, 165), (2, 256)])
def test_bert_sampler_equals_the_restatement(dev, B, S):
    from clibd_amd import mlm, ops

    V = 1027
    g = torch.Generator().manual_seed(S)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(0, V, (B, S - 1), generator=g)], dim=1)     # special ids inside
    mask = (torch.rand(B, S, generator=g) > 0.25).long()
    for am in (None, mask):
        for seed, p, replace in ((31337, 0.15, (0.8, 0.1, 0.1)), (0x80000001, 0.5, (0.8, 0.1, 0.1)), (0xFFFFFFFF, 1.0, (0.5, 0.5, 0.0)),
                                 (5, 0.5, (1.0, 0.0, 0.0)), (6, 0.0, (0.8, 0.1, 0.1))):
            want = LR.sample_bert(ids.numpy(), None if am is None else am.numpy(), V, seed, p=p, replace=replace)
            got = ops.mlm_mask_bert(ids.to(dev), None if am is None else am.to(dev), V, seed, p, 0, (0, 1, 2), replace)
            again = ops.mlm_mask_bert(ids.to(dev), None if am is None else am.to(dev), V, seed, p, 0, (0, 1, 2), replace)
            for w, x, y, name in zip(want, got, again, ("masked", "labels")):
                assert x.dtype == torch.int64 and np.array_equal(x.cpu().numpy(), w), (name, seed, am is None)
                assert torch.equal(x, y)
    torch.manual_seed(5)
    a = mlm.mask_tokens_bert(ids.to(dev), mask.to(dev), vocab_size=V)
    torch.manual_seed(5)
    b = mlm.mask_tokens_bert(ids.to(dev), mask.to(dev), vocab_size=V)            # seed=None: the CPU generator, reproducible
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].shape == (B, S)


# ---- 3. gather and scatter with padding rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("r_cap", [64, 192])
def test_gather_and_scatter_with_padding_rows(dev, H, r_cap):
    from clibd_amd import ops

    M, n = 333, r_cap - 23
    g = torch.Generator().manual_seed(H + r_cap)
    x = torch.randn(M, H, generator=g).to(BF16)
    rows = torch.full((r_cap,), ops.MLM_PAD_ROW, dtype=torch.int32)
    rows[:n] = torch.randperm(M, generator=g)[:n].sort().values.to(torch.int32)
    got = ops.rows_gather(x.to(dev), rows.to(dev)).cpu()
    assert torch.equal(got[:n], x[rows[:n].long()]) and (got[n:].view(torch.int16) == 0).all()            # padding rows read zeros
    src = torch.randn(r_cap, H, generator=g).to(BF16)
    src[n:] = float("nan")                                                                                 # a padding row must never land anywhere
    out = torch.full((M + 2, H), float("nan"), dtype=BF16, device=dev)                                     # guard rows on both sides
    ops.rows_scatter(src.to(dev), rows.to(dev), M, out=out[1:M + 1])
    want = torch.zeros(M, H, dtype=BF16)
    want[rows[:n].long()] = src[:n]
    out = out.cpu()
    assert torch.equal(out[1:M + 1].view(torch.int16), want.view(torch.int16)) and out[0].isnan().all() and out[M + 1].isnan().all()


# ---- 4. equivalence with the existing path -------------------------------------------------------------------------------------------------------
def test_labels_form_equals_the_rows_form_bit_for_bit(dev):
    """B = 8, S = 33, mask_ratio 0.5: 8 x 16 = 128 rows, a multiple of 64, so the capacity can equal the count"""
    from clibd_amd import mlm

    B, S, V = 8, 33, A["vocab_size"]
    g = torch.Generator().manual_seed(12)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1).to(dev)
    m = pretraining_model(A, tied_state(321, A), True, dev).eval().set_deterministic(True)
    masked, rows, targets, n_valid = mlm.mask_tokens(ids, 0.5, seed=99)
    assert rows.numel() == 128 and int(n_valid) == 128
    labels = torch.full((B * S,), LR.IGNORE, dtype=torch.int64, device=dev)
    labels[rows.long()] = targets
    labels = labels.view(B, S)
    ones = torch.ones(B, S, dtype=torch.int64, device=dev)
    loss0, correct0 = m(masked, rows, targets, n_valid)
    g0 = grads_by_key(m, loss0)
    loss1, correct1 = m(input_ids=masked, attention_mask=ones, labels=labels, label_capacity=128)
    g1 = grads_by_key(m, loss1)
    assert torch.equal(loss1.detach(), loss0.detach()) and torch.equal(correct1, correct0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    # 64 padding rows more: the gates of the golden test, against the existing call
    loss2, correct2 = m(input_ids=masked, attention_mask=ones, labels=labels, label_capacity=192)
    g2 = grads_by_key(m, loss2)
    print(f"capacity 192 against 128: loss {float(loss2.detach()):.7f} / {float(loss0.detach()):.7f}")
    assert abs(float(loss2.detach()) - float(loss0.detach())) < 1e-3 and torch.equal(correct2, correct0)
    assert_grads(g2, g0, rel_tol=3e-2, cos_tol=0.999, what="capacity 192 vs 128", zero_tol=2e-6, zero_rel=1e-4)
    assert int(m.label_overflow) == 0
    # the gradient of the top hidden state: the head alone, on one top state, at both capacities
    x_top = torch.randn(B * S, A["hidden_size"], generator=torch.Generator().manual_seed(3)).to(BF16).to(dev)
    one = torch.ones((), dtype=torch.float32, device=dev)
    dxs = []
    for cap in (128, 192):
        r, t, n = mlm.ops.mlm_compact_labels(labels, V, cap)
        _, _, head = m._head_forward(x_top, r, t, n)
        sink = {id(p): torch.zeros_like(p, dtype=torch.float32) for p in m.cls.predictions.parameters()}
        dxs.append(m._head_backward(one, head, sink))
    want_zero = torch.ones(B * S, dtype=torch.bool)
    want_zero[rows.long().cpu()] = False
    assert torch.equal(dxs[0], dxs[1]) and float(dxs[0].float().abs().max()) > 0 and (dxs[1].cpu()[want_zero] == 0).all()


# ---- 5. against the HF golden and the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("name", [c[0] for c in LR.CASES])
def test_loss_and_gradients_match_hf_golden_and_oracle(dev, golden, name, tied):
    """the bounds of tests/test_mlm_gpu.py::test_loss_and_gradients_match_golden_and_oracle (its lines 205-223), number for number"""
    from oracle import clibd_oracle as O

    g = golden[(name, tied)]
    sd = tied_state(g["seed"], g["config"], tied)
    assert MR.state_hash(sd) == g["weights_sha256"]
    m = pretraining_model(g["config"], sd, tied, dev).eval()
    ids, mask, labels = g["input_ids"], g["attention_mask"], g["labels"]
    loss, correct = m(input_ids=ids.to(dev), attention_mask=mask.to(dev), labels=labels.to(dev))
    got = grads_by_key(m, loss)
    om = MR.oracle_for(g["config"], sd, tied)
    with O.precision("bf16"):
        lo, hits = LR.labels_loss(om, ids, mask, labels)
        go = MR.named_grads(om, lo)
    print(f"{name} tied={tied}: loss device {float(loss.detach()):.6f}, oracle bf16 {float(lo.detach()):.6f}, HF fp32 {g['loss']:.6f}; hits {int(correct)} / {hits} / {g['hits']}")
    assert abs(float(loss.detach()) - float(lo.detach())) < 1e-3
    assert_grads(got, go, rel_tol=3e-2, cos_tol=0.999, what=f"mlm labels {name} tied={tied} vs oracle-bf16", zero_tol=2e-6, zero_rel=1e-4)
    assert abs(int(correct) - hits) <= 1
    assert abs(float(loss.detach()) - g["loss"]) < 2e-2 * abs(g["loss"])
    assert_grads({k: MR.sampled(k, v) for k, v in got.items()}, g["grads"], rel_tol=5e-2, cos_tol=0.998, what=f"mlm labels {name} tied={tied} vs HF fp32",
                 zero_tol=2e-6, zero_rel=1e-4)
    gmax = max(g["grad_norms"].values())
    for k, n in g["grad_norms"].items():
        if n > 1e-4 * gmax:
            assert abs(float(got[k].double().norm()) - n) < 5e-2 * n, (k, float(got[k].double().norm()), n)
    if tied:
        assert torch.equal(got["cls.predictions.decoder.weight"], got["bert.embeddings.word_embeddings.weight"])
    else:
        assert float(got["cls.predictions.bias"].abs().max()) == 0.0
    with torch.no_grad():
        l2, c2 = m(input_ids=ids.to(dev), attention_mask=mask.to(dev), labels=labels.to(dev), label_capacity=pad64(g["n_labelled"]))
    assert not l2.requires_grad and abs(float(l2) - g["loss"]) < 2e-2 * abs(g["loss"]) and abs(int(c2) - g["hits"]) <= 1
    assert int(m.label_overflow) == 0


# ---- 6. train mode, deterministic mode -----------------------------------------------------------------------------------------------------------
def _ragged(B, S, V, seed, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1)
    mask = torch.ones(B, S, dtype=torch.long)
    for b in range(B):
        n = S if b % 3 == 0 else 2 + (b * 7) % (S - 2)
        mask[b, n:] = 0
        ids[b, n:] = 2
    return ids.to(dev), mask.to(dev)


def _bert_steps(dev, steps):
    from clibd_amd import mlm
    from clibd_amd.optim import FusedAdamW

    m = pretraining_model(A, tied_state(55, A), True, dev).train().set_deterministic(True)          # dropout 0.1, as configured
    opt = FusedAdamW(m.parameters(), lr=1e-3)
    m.attach(opt)
    ids, mask = _ragged(6, 33, A["vocab_size"], 4, dev)
    torch.manual_seed(77)                         # the sampler's seed and the dropout base come from the CPU generator
    out = None
    for _ in range(steps):
        out = mlm.pretrain_step(m, (ids, mask), opt, sampler="bert", mlm_probability=0.3)
    return m, opt, out


def test_train_mode_step_with_mask_dropout_and_bert_sampler(dev):
    from clibd_amd import mlm

    m = pretraining_model(A, tied_state(55, A), True, dev).train()
    ids, mask = _ragged(6, 33, A["vocab_size"], 4, dev)
    masked, labels = mlm.mask_tokens_bert(ids, mask, 0.3, seed=8, vocab_size=m)
    assert int((labels != LR.IGNORE).sum()) > 10 and not (labels != LR.IGNORE)[mask == 0].any()
    torch.manual_seed(3)
    loss, _ = m(input_ids=masked, attention_mask=mask, labels=labels)
    got = grads_by_key(m, loss)
    m.eval()
    with torch.no_grad():
        le, _ = m(input_ids=masked, attention_mask=mask, labels=labels)
    assert torch.isfinite(loss) and float(loss.detach()) != float(le)         # the dropout masks did something
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        if not k.endswith("attention.self.key.bias"):                  # analytically zero: softmax ignores a per-query constant
            assert float(v.abs().max()) > 0, k
    (m1, o1, r1), (m2, o2, r2) = _bert_steps(dev, 2), _bert_steps(dev, 2)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2)) and torch.isfinite(r1[0]) and 0 < int(r1[2]) < 6 * 33
    assert torch.equal(o1.flat_g, o2.flat_g) and torch.equal(o1.flat_p, o2.flat_p) and float(o1.flat_g.abs().max()) > 0
    assert int(m1.label_overflow) == 0


# ---- 7. padding has no influence ---------------------------------------------------------------------------------------------------------------
def test_ids_at_masked_out_unlabelled_positions_change_nothing(dev):
    from clibd_amd import mlm

    V = A["vocab_size"]
    m = pretraining_model(A, tied_state(56, A), True, dev).eval().set_deterministic(True)
    ids, mask = _ragged(6, 33, V, 9, dev)
    masked, labels = mlm.mask_tokens_bert(ids, mask, 0.3, seed=21, vocab_size=m)
    dead = mask == 0
    assert int(dead.sum()) > 20 and (labels[dead] == LR.IGNORE).all()
    other = masked.clone()
    other[dead] = torch.randint(3, V, (int(dead.sum()),), generator=torch.Generator().manual_seed(1)).to(dev)
    l0, c0 = m(input_ids=masked, attention_mask=mask, labels=labels)
    g0 = grads_by_key(m, l0)
    l1, c1 = m(input_ids=other, attention_mask=mask, labels=labels)
    g1 = grads_by_key(m, l1)
    assert torch.equal(l0.detach(), l1.detach()) and torch.equal(c0, c1)
    touched = torch.unique(torch.cat([masked[dead], other[dead]])).cpu()       # the embedding rows of the changed ids: their positions feed nothing
    keep = torch.ones(V, dtype=torch.bool)
    keep[touched] = False
    for k in g0:
        if k in ("bert.embeddings.word_embeddings.weight", "cls.predictions.decoder.weight"):
            assert torch.equal(g0[k][keep], g1[k][keep]), k
        else:
            assert torch.equal(g0[k], g1[k]), k
    # and the mask itself matters: without it the padded keys are attended and the loss moves
    l2, _ = m(input_ids=masked, labels=labels)
    assert float(l2.detach()) != float(l0.detach())


# ---- 8. it learns --------------------------------------------------------------------------------------------------------------------------------
def test_fixed_batch_is_learned_through_the_bert_sampler(dev):
    """tests/test_mlm_gpu.py::test_fixed_batch_is_learned_as_in_the_fp32_oracle through pretrain_step(sampler="bert") with a ragged mask:
    the recipe of mlm_reference.LEARN with mlm_labels_reference.learn_inputs' mask and one fixed draw of the sampler (p = 0.3, 59 labelled
    positions).  The fp32 oracle on the CPU (mlm_labels_reference.oracle_learning_curve): initial loss 5.689, half of it passed at step
    13, 0.414 after 40 steps, 0.102 after 60.  That test's criterion: the first loss within 2 % of the oracle's, and after 40 steps
    below half of the oracle's initial loss.  The mark is the oracle's, not this code's."""
    from clibd_amd import mlm
    from clibd_amd.optim import FusedAdamW

    ORACLE_INITIAL, STEPS = 5.689, 40
    cfg = MR.LEARN["config"]
    m = pretraining_model(cfg, tied_state(MR.LEARN["seed"], cfg), True, dev).train()
    opt = FusedAdamW(m.parameters(), lr=MR.LEARN["lr"], weight_decay=MR.LEARN["weight_decay"])
    m.attach(opt)
    ids, mask, masked, labels = LR.learn_inputs()
    ids, mask = ids.to(dev), mask.to(dev)
    got = mlm.mask_tokens_bert(ids, mask, LR.LEARN_P, seed=LR.LEARN_SEED, vocab_size=m)
    assert torch.equal(got[0].cpu(), masked) and torch.equal(got[1].cpu(), labels)
    losses = []
    for _ in range(STEPS):
        loss, _, n = mlm.pretrain_step(m, (ids, mask), opt, seed=LR.LEARN_SEED, sampler="bert", mlm_probability=LR.LEARN_P)
        losses.append(loss)
    m.eval()
    with torch.no_grad():
        final, correct = m(input_ids=masked.to(dev), attention_mask=mask, labels=labels.to(dev))
    curve = torch.stack(losses).tolist()
    print(f"learning: device loss {curve[0]:.3f} -> {float(final):.3f} after {STEPS} steps (oracle fp32: 5.689 -> 0.414); hits {int(correct)} of {int(n)}")
    assert int(n) == int((labels != LR.IGNORE).sum()) == 59
    assert abs(curve[0] - ORACLE_INITIAL) < 2e-2 * ORACLE_INITIAL
    assert float(final) < 0.5 * ORACLE_INITIAL
    assert int(m.label_overflow) == 0


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_wide_heads_refuse_a_mask_and_take_labels_without_one(dev):
    from clibd_amd import mlm
    from clibd_amd.engine import NotSupportedYet

    B, S, V = 4, 33, WIDE["vocab_size"]
    m = pretraining_model(WIDE, tied_state(57, WIDE), True, dev).eval().set_deterministic(True)          # 128-wide heads
    g = torch.Generator().manual_seed(13)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=g)], dim=1).to(dev)
    masked, labels = mlm.mask_tokens_bert(ids, None, 0.5, seed=3, vocab_size=V)
    with pytest.raises(NotSupportedYet, match="attention mask"):
        m(input_ids=masked, attention_mask=torch.ones_like(ids), labels=labels)
    with pytest.raises(NotSupportedYet, match="attention mask"):
        m(*mlm.mask_tokens(ids, 0.5, seed=3), attention_mask=torch.ones_like(ids))
    loss, correct = m(input_ids=masked, labels=labels)
    got = grads_by_key(m, loss)
    assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in got.values()) and float(got["cls.predictions.transform.dense.weight"].abs().max()) > 0
    with pytest.raises(TypeError):
        m(masked, labels=labels)
    with pytest.raises(TypeError):
        m(input_ids=masked)
    with pytest.raises(ValueError):
        m(input_ids=masked, labels=labels[:, :-1])


def test_overflow_makes_pretrain_epoch_raise(dev):
    from clibd_amd import mlm
    from clibd_amd.optim import FusedAdamW

    m = pretraining_model(A, tied_state(58, A), True, dev)
    opt = FusedAdamW(m.parameters(), lr=1e-3)
    ids, mask = _ragged(6, 33, A["vocab_size"], 5, dev)
    torch.manual_seed(1)
    stats = mlm.pretrain_epoch(m, [(ids, mask), ids], opt, sampler="bert", mlm_probability=0.15)          # the default capacity suffices
    assert stats["steps"] == 2 and 0 < stats["loss"] < 20 and 0 <= stats["accuracy"] <= 1
    with pytest.raises(RuntimeError, match="label_capacity"):
        mlm.pretrain_epoch(m, [ids], opt, sampler="bert", mlm_probability=0.9, label_capacity=64)          # ~170 labelled positions
    assert int(m.label_overflow) == 0                                                                        # re-armed
    with pytest.raises(ValueError, match="sampler"):
        mlm.pretrain_step(m, ids, opt, sampler="span")
