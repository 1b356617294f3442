"""GPU checks of the linear-probe classifier: the kernels of csrc/classifier.hip (head at split-bf16 accuracy, cross-entropy, softmax top-k)
against fp64 restatements, their edges, the accuracy claim the split product is there for, and clibd_amd.method_linear against the
reference's recorded results (tests/golden/method_linear_golden.pt, made by tests/golden/make_method_linear_golden.py).  The gates of the
kernels are the project's own for the same operand technique (tests/test_ops_gpu.py::test_softce_rows_fwd_bwd, tests/test_simclr_gpu.py):
|loss - ref| < 2e-4 |ref| + 1e-3, rel_err < 1e-4 for logits, dx, dw and db each.

Measured on an MI355X (the figures these tests print; GAP = 2e-5 is the fixture's decision margin):
  max |logit - fp64| 1.4e-5 (C = 2, |logit| <= 1.6), 1.7e-5 (the golden head, |logit| <= 6.5) .. 6.3e-5 (C = 916, D = 768, |logit| <= 14.6);
  max |conf - fp64| 1.7e-6 .. 8.0e-6 over the seven shapes, 3.0e-6 on the golden; rel_err of logits, dx, dw, db 1.8e-6 .. 8.8e-6;
  on the golden features and head: max |conf - reference fp32| 3.0e-6 with every index equal, against 1.9e-3 for one plain bf16 GEMM;
  72 fine-tuning steps: max |loss - reference| 1.2e-6."""
import functools
import importlib.util
import types
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
LEVELS = ["order", "family", "genus", "species"]
SHAPES = [(1, 2, 64), (3, 5, 64), (4, 64, 64), (5, 65, 128), (33, 36, 128), (33, 916, 768), (257, 916, 768)]


def rel_err(a, b):      # as in tests/test_ops_gpu.py
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def loss_close(got, ref):
    return abs(got - ref) < 2e-4 * abs(ref) + 1e-3


@functools.lru_cache(maxsize=None)
def _gen():
    spec = importlib.util.spec_from_file_location("make_method_linear_golden", ROOT / "tests" / "golden" / "make_method_linear_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _golden():
    return torch.load(ROOT / "tests" / "golden" / "method_linear_golden.pt", weights_only=False)


@pytest.fixture(scope="module")
def golden():
    return _golden()


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def ML(dev):
    from clibd_amd import method_linear

    return method_linear


def fp64_ref(x, w, b, t, k):
    """torch fp64 on the CPU: logits, mean cross-entropy, dx, dw, db at upstream gradient 1, conf / idx of topk(softmax)"""
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    logits = F.linear(xd, wd, bd)
    loss = F.cross_entropy(logits, t)
    dx, dw, db = torch.autograd.grad(loss, (xd, wd, bd))
    conf, idx = torch.topk(F.softmax(logits.detach(), dim=-1), k, dim=1, largest=True, sorted=True)
    return dict(logits=logits.detach(), loss=loss.item(), dx=dx, dw=dw, db=db, conf=conf, idx=idx)


@functools.lru_cache(maxsize=None)
def case(B, C, D):
    """(x, w, b, target, fp64 reference), computed once per shape.  (33, 36, 128) is the golden's kernel case: the first 33 seen queries,
    the trained head, their classes.  Elsewhere unit rows against a random head whose logits have a standard deviation of about 3;
    the targets include class 0 and class C - 1."""
    if (B, C, D) == (33, 36, 128):
        g, G = _golden(), _gen()
        x = torch.from_numpy(G.synth("seen_query", g["redraw"]["seen_query"])[0][:33].copy())
        w, b = torch.from_numpy(g["head"]["weight"].copy()), torch.from_numpy(g["head"]["bias"].copy())
        t = torch.from_numpy(g["kernel"]["target"].copy())
    else:
        gen = torch.Generator().manual_seed(100000 * B + 100 * C + D)
        x = F.normalize(torch.randn(B, D, generator=gen), dim=-1)
        w = torch.randn(C, D, generator=gen) * 3.0              # unit rows: logits ~ N(0, 3^2)
        b = torch.randn(C, generator=gen) * 0.5
        t = torch.randint(0, C, (B,), generator=gen)
        t[0] = C - 1
        if B > 1:
            t[1] = 0
    return x, w, b, t, fp64_ref(x, w, b, t, min(5, C))


def run(ops, dev, x, w, b, t, dloss=None, k=5):
    xd, wd, bd, td = x.to(dev), w.to(dev), b.to(dev), t.to(dev)
    logits = ops.linear_f32_fwd(xd, wd, bd)
    loss, lse = ops.ce_rows_fwd(logits, td)
    d = ops.ce_rows_bwd(logits, td, lse, None if dloss is None else torch.tensor([dloss], device=dev))
    dx, dw, db = ops.linear_f32_bwd(d, xd, wd)
    conf, idx = ops.softmax_topk(logits, min(k, w.shape[0]))
    torch.cuda.synchronize()
    return dict(logits=logits.cpu(), loss=loss.item(), lse=lse.cpu(), dlogits=d.cpu(), dx=dx.cpu(), dw=dw.cpu(), db=db.cpu(), conf=conf.cpu(), idx=idx.cpu())


# ------------------------------------------------------------------------------------------------------------- kernels against fp64
# (1, 2, 64): minimal; (3, 5, 64): a row shorter than a wave; (4, 64, 64): exactly one lane stride; (5, 65, 128): one element past it;
# (33, 36, 128): the golden; (33, 916, 768): the reference's classes, C a multiple of neither 16 nor 64; (257, 916, 768): B crosses a
# 256-row tile, ragged tiles in both backward products
@pytest.mark.parametrize("B,C,D", SHAPES)
def test_kernels_against_fp64(ops, dev, golden, B, C, D):
    x, w, b, t, ref = case(B, C, D)
    assert int(t.min()) == 0 or B == 1
    assert int(t.max()) == C - 1 or (B, C, D) == (33, 36, 128)
    got = run(ops, dev, x, w, b, t)
    k = min(5, C)
    print(f"(B, C, D) = ({B}, {C}, {D}): max |logit - fp64| {(got['logits'].double() - ref['logits']).abs().max().item():.3e} "
          f"(max |logit| {ref['logits'].abs().max().item():.2f}), max |conf - fp64| {(got['conf'].double() - ref['conf']).abs().max().item():.3e}, "
          f"loss {got['loss']:.7f} ref {ref['loss']:.7f}, rel_err logits {rel_err(got['logits'], ref['logits']):.2e} dx {rel_err(got['dx'], ref['dx']):.2e} "
          f"dw {rel_err(got['dw'], ref['dw']):.2e} db {rel_err(got['db'], ref['db']):.2e}")
    assert loss_close(got["loss"], ref["loss"]), (got["loss"], ref["loss"])
    for name in ("logits", "dx", "dw", "db"):
        assert rel_err(got[name], ref[name]) < 1e-4, (name, rel_err(got[name], ref[name]))
    assert got["conf"].shape == (B, k) and got["idx"].dtype == torch.int64
    assert (got["conf"].double() - ref["conf"]).abs().max().item() < 1e-5
    if (B, C, D) == (33, 36, 128):      # the recorded fp64 values of the fixture, and its margins: every index equal
        kk = golden["kernel"]
        assert loss_close(got["loss"], kk["loss"])
        for name in ("logits", "dx", "dw", "db"):
            assert rel_err(got[name], torch.from_numpy(kk[name])) < 1e-4, name
        assert torch.equal(got["idx"], ref["idx"])
        assert torch.equal(got["idx"], torch.from_numpy(golden["idx"]["seen_query"][:33].astype(np.int64)))
    # an upstream gradient scales every gradient: one more fp32 factor ahead of the same products
    got2 = run(ops, dev, x, w, b, t, dloss=0.37)
    assert got2["loss"] == got["loss"]
    assert ((got2["dlogits"].double() - 0.37 * got["dlogits"].double()).abs() <= 1e-6 * got["dlogits"].double().abs() + 1e-37).all()
    for name in ("dx", "dw", "db"):
        assert rel_err(got2[name], 0.37 * ref[name]) < 1e-4, name


def test_strided_logits_and_scalar_path(ops, dev):
    """logits with a leading dimension that is no multiple of 4 take the scalar loads, an aligned one the 16-byte loads: the same values"""
    x, w, b, t, ref = case(5, 65, 128)
    xd, wd, bd, td = x.to(dev), w.to(dev), b.to(dev), t.to(dev)
    wide = torch.full((5, 67), float("nan"), device=dev)
    ops.linear_f32_fwd(xd, wd, bd, out=wide[:, :65])
    dense = ops.linear_f32_fwd(xd, wd, bd)
    pad4 = torch.full((5, 68), float("nan"), device=dev)
    pad4[:, :65] = dense
    assert torch.equal(wide[:, :65], dense) and torch.isnan(wide[:, 65:]).all()
    outs = [(ops.ce_rows_fwd(v, td), ops.softmax_topk(v, 5)) for v in (wide[:, :65], dense, pad4[:, :65])]
    torch.cuda.synchronize()
    for (loss, lse), (conf, idx) in outs:
        assert loss_close(loss.item(), ref["loss"])
        assert torch.allclose(lse, outs[0][0][1], rtol=0, atol=4e-6)      # another summation order: a few ulp of lse ~ 10
        assert torch.equal(idx, outs[0][1][1]) and torch.equal(conf, outs[0][1][0])
    d = ops.ce_rows_bwd(wide[:, :65], td, outs[0][0][1])
    assert torch.equal(d, ops.ce_rows_bwd(dense, td, outs[0][0][1]))


# ------------------------------------------------------------------------------------------------------------------------------ edges
def test_large_logits_stay_finite(ops, dev):
    """A row whose logits sit near +200 and one entry +100 above the rest: exp overflows fp32 without the running maximum.  The loss and
    the gradients are finite and follow fp64; confidences that underflow to 0 are compared by value only."""
    gen = torch.Generator().manual_seed(11)
    B, C = 6, 70
    logits = torch.randn(B, C, generator=gen)
    logits[1] += 200.0
    logits[2, 17] += 100.0
    logits[3] += 200.0
    logits[3, 69] += 100.0
    t = torch.tensor([3, 5, 17, 69, 0, 69])
    ld = logits.double().requires_grad_(True)
    ref_loss = F.cross_entropy(ld, t)
    (ref_d,) = torch.autograd.grad(ref_loss, ld)
    rc, ri = torch.topk(F.softmax(logits.double(), dim=-1), 8, dim=1)
    lg = logits.to(dev)
    loss, lse = ops.ce_rows_fwd(lg, t.to(dev))
    d = ops.ce_rows_bwd(lg, t.to(dev), lse)
    conf, idx = ops.softmax_topk(lg, 8)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(lse).all() and torch.isfinite(d).all() and torch.isfinite(conf).all()
    assert loss_close(loss.item(), ref_loss.item()), (loss.item(), ref_loss.item())
    assert (d.cpu().double() - ref_d).abs().max().item() < 1e-5 / B * 10
    assert (conf.cpu().double() - rc).abs().max().item() < 1e-5
    assert (conf.cpu()[2, 1:] < 1e-40).all() and conf.cpu()[2, 0] == 1.0      # e^-100 is below fp32's normal range: values only
    live = rc > 1e-30
    assert torch.equal(idx.cpu()[live], ri[live])


@pytest.mark.parametrize("k", [1, 5, 8, "C"])
def test_softmax_topk_k_and_ties(ops, dev, k):
    """k = 1, 5, 8 and k = C against torch; equal values resolve to the lower index (torch.topk leaves the order of ties open)"""
    gen = torch.Generator().manual_seed(12)
    for B, C in ((7, 8), (5, 200), (3, 1000)):
        kk = min(C, 8) if k == "C" else k
        if k == "C" and C > 8:
            continue
        logits = torch.randn(B, C, generator=gen) * 3
        rc, ri = torch.topk(F.softmax(logits.double(), dim=-1), kk, dim=1)
        conf, idx = ops.softmax_topk(logits.to(dev), kk)
        assert torch.equal(idx.cpu(), ri) and (conf.cpu().double() - rc).abs().max().item() < 1e-6
        assert (conf.cpu()[:, :-1] >= conf.cpu()[:, 1:]).all()
    # ties: every value four times, spread over lanes and over one lane's own list (indices j, j + 64, ...)
    C = 300
    base = torch.randn(75, generator=gen).repeat(4)[torch.randperm(C, generator=gen)]
    logits = base[None, :].repeat(2, 1)
    kk = 8 if k == "C" else k
    conf, idx = ops.softmax_topk(logits.to(dev), kk)
    order = sorted(range(C), key=lambda j: (-base[j].item(), j))[:kk]
    assert idx.cpu()[0].tolist() == order and idx.cpu()[1].tolist() == order
    # all equal: indices 0 .. k - 1, confidence 1 / C
    conf, idx = ops.softmax_topk(torch.zeros(3, 130, device=dev), kk)
    assert idx.cpu()[1].tolist() == list(range(kk)) and torch.allclose(conf.cpu(), torch.full((3, kk), 1.0 / 130))


def test_softmax_topk_k_beyond_classes_raises(ops, dev):
    with pytest.raises(RuntimeError):
        ops.softmax_topk(torch.zeros(2, 4, device=dev), 5)
    for k in (0, 9):
        with pytest.raises(ValueError):
            ops.softmax_topk(torch.zeros(2, 40, device=dev), k)
    from clibd_amd import _lib

    logits = torch.zeros(2, 4, device=dev)
    conf, idx = torch.zeros(2, 5, device=dev), torch.zeros(2, 5, dtype=torch.int64, device=dev)
    assert _lib.load().clibd_softmax_topk(logits.data_ptr(), 4, 2, 4, 5, conf.data_ptr(), idx.data_ptr(), None) == -1


@pytest.mark.parametrize("bad", [-1, "C", -100])
def test_target_outside_the_classes(ops, dev, bad):
    """A target of -1 or C (or torch's ignore_index): its row's gradient is zero, the loss is the other rows' sum over B, bit 0 of the error
    word is set.  The kernel reads nothing for such a target."""
    x, w, b, t, ref = case(5, 65, 128)
    C = 65
    logits = ref["logits"].float()
    t = t.clone()
    t[2] = C if bad == "C" else bad
    lp = F.log_softmax(ref["logits"], dim=-1)
    keep = [i for i in range(5) if i != 2]
    ref_loss = -sum(lp[i, t[i]].item() for i in keep) / 5
    lg, td = logits.to(dev), t.to(dev)
    err = ops.ce_error_word(dev)
    err.zero_()
    loss, lse = ops.ce_rows_fwd(lg, td)
    d = ops.ce_rows_bwd(lg, td, lse)
    torch.cuda.synchronize()
    assert int(err.item()) & 1
    assert loss_close(loss.item(), ref_loss) and abs(loss.item() - ref_loss) < 1e-5
    assert (d[2] == 0).all() and (d[keep].abs().sum(dim=1) > 0).all()
    with pytest.raises(ValueError):
        ops.ce_rows_fwd(lg, td, check=True)
    assert int(err.item()) == 0                                      # read back and cleared
    t[2] = 7
    ops.ce_rows_fwd(lg, t.to(dev), check=True)
    assert int(err.item()) == 0


def test_two_calls_are_bit_identical(ops, dev):
    x, w, b, t, _ = case(257, 916, 768)
    a, c = run(ops, dev, x, w, b, t), run(ops, dev, x, w, b, t)
    for name in ("loss", "dx", "dw", "db", "conf", "idx", "logits", "dlogits"):
        same = a[name] == c[name] if name == "loss" else torch.equal(a[name], c[name])
        assert same, name


# --------------------------------------------------------------------------------------------------------------- the accuracy claim
def _query_features(golden):
    G = _gen()
    return {s: torch.from_numpy(G.synth(s, golden["redraw"][s])[0].copy()) for s in ("seen_query", "unseen_query")}


def test_split_product_keeps_the_fixture_margin_and_plain_bf16_does_not(ops, dev, golden):
    """On the golden features and head: max |conf - reference fp32| < GAP / 2 with every index equal; the same inputs through ONE plain
    bf16 GEMM (ops.gemm_nt on bf16 casts) miss the reference by more than GAP — why the head runs on split operands."""
    gap = golden["gap"]
    feats = _query_features(golden)
    w, b = torch.from_numpy(golden["head"]["weight"]).to(dev), torch.from_numpy(golden["head"]["bias"]).to(dev)
    w48 = torch.zeros(48, 128, device=dev)
    w48[:36] = w
    b48 = torch.zeros(48, device=dev)
    b48[:36] = b
    worst_split = worst_plain = 0.0
    for s, x in feats.items():
        ref_conf = torch.from_numpy(golden["conf"][s])
        ref_idx = torch.from_numpy(golden["idx"][s].astype(np.int64))
        conf, idx = ops.softmax_topk(ops.linear_f32_fwd(x.to(dev), w, b), 5)
        assert torch.equal(idx.cpu(), ref_idx), s
        worst_split = max(worst_split, (conf.cpu().double() - ref_conf.double()).abs().max().item())
        plain = torch.empty(x.shape[0], 48, device=dev)
        ops.gemm_nt(x.to(dev).to(torch.bfloat16), w48.to(torch.bfloat16), bias=b48, out_f32=plain)
        pc, _ = ops.softmax_topk(plain[:, :36], 5)
        worst_plain = max(worst_plain, (pc.cpu().double() - ref_conf.double()).abs().max().item())
    print(f"golden features and head: max |conf - reference fp32| split product {worst_split:.3e}, one plain bf16 GEMM {worst_plain:.3e} (GAP {gap:.1e})")
    assert worst_split < gap / 2, worst_split
    assert worst_plain > gap, worst_plain


# ------------------------------------------------------------------------------------------------------------------------- modules
def test_autograd_modules_agree_with_the_direct_calls(ops, ML, dev):
    x, w, b, t, ref = case(33, 916, 768)
    direct = run(ops, dev, x, w, b, t, dloss=0.37)
    xd = x.to(dev).requires_grad_(True)
    model = ML.ViTWIthExtraLayer(torch.nn.Identity(), torch.nn.Linear(768, 916)).to(dev)
    with torch.no_grad():
        model.new_linear_layer.weight.copy_(w)
        model.new_linear_layer.bias.copy_(b)
    out = model(xd)
    loss = ML.CrossEntropyLoss()(out, t.to(dev))
    (loss * 0.37).backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and loss.item() == direct["loss"]
    assert torch.equal(out.detach().cpu(), direct["logits"])
    assert torch.equal(xd.grad.cpu(), direct["dx"])
    assert torch.equal(model.new_linear_layer.weight.grad.cpu(), direct["dw"]) and torch.equal(model.new_linear_layer.bias.grad.cpu(), direct["db"])
    assert torch.equal(model.get_feature(xd), xd)
    # a drop-in: the reference's `criterion(output, target)` against torch's own on the same logits
    assert abs(loss.item() - F.cross_entropy(out.detach().double().cpu(), t).item()) < 1e-5


def _loaders(golden, dev):
    G = _gen()
    g = golden
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    feats = {s: G.synth(s, g["redraw"].get(s)) for s in G.SPLITS}
    img = {s: G.loader_of(s, feats[s][0], g["batch"] if s == "train_seen" else g["query_batch"], to_dev) for s in G.SPLITS}
    return G, feats, img


class _FeatureModel(torch.nn.Module):
    """the 'original model' of the synthetic world: a loader's image batch holds image features, its dna batch DNA features"""

    image_encoder = dna_encoder = True
    language_encoder = None

    def forward(self, image, dna, language):
        return image, dna, None


def _with_dna(loader, dna, dev):
    out, r = [], 0
    for b in loader:
        n = len(b[0])
        out.append((b[0], b[1], torch.from_numpy(np.ascontiguousarray(dna[r:r + n])).to(dev), None, None, None, b[6]))
        r += n
    return out


def test_fine_tuning_losses_follow_the_reference(ML, dev, golden):
    """fine_tuning_epoch with the identity encoder on the golden batches, from the recorded initial head, FusedAdamW + OneCycleLR at the
    generator's settings: every step's loss within the loss gate of the reference's, and the loss falls."""
    from torch.optim.lr_scheduler import OneCycleLR

    from clibd_amd.optim import FusedAdamW

    g = golden
    G, _, img = _loaders(g, dev)
    head = torch.nn.Linear(128, 36)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(g["head0"]["weight"]))
        head.bias.copy_(torch.from_numpy(g["head0"]["bias"]))
    model = ML.ViTWIthExtraLayer(torch.nn.Identity(), head).to(dev)
    opt = FusedAdamW(model.parameters(), lr=g["lr"])
    sched = OneCycleLR(opt, max_lr=g["lr"], total_steps=len(img["train_seen"]) * g["epochs"])
    steps, epoch_losses = [], []
    for _ in range(g["epochs"]):
        el, ev = ML.fine_tuning_epoch(None, model, img["train_seen"], None, None, opt, ML.CrossEntropyLoss(), sched, dev, g["label_map"], step_losses=steps)
        epoch_losses.append(el)
        assert ev is None
    got = torch.stack(steps).cpu().double().numpy()
    ref = g["step_losses"]
    worst = np.abs(got - ref).max()
    print(f"{len(ref)} steps: loss {got[0]:.5f} -> {got[-1]:.5f} (reference {ref[0]:.5f} -> {ref[-1]:.5f}), max |loss - reference| {worst:.3e}")
    assert got.shape == ref.shape
    assert (np.abs(got - ref) < 2e-4 * np.abs(ref) + 1e-3).all(), worst
    assert got[-1] < 0.1 * got[0]
    assert np.allclose(epoch_losses, g["epoch_losses"], rtol=0, atol=2e-4 * ref.max() + 1e-3)      # a mean of steps that each hold the gate
    ev = ML.evaluate_epoch(model, img["seen_query"], dev, g["label_map"])
    assert set(ev) == {"top1_accuracy", "top3_accuracy", "top5_accuracy"} and not model.training


def _unpack(codes, vocab):
    return [{lv: [vocab[l][c] for c in row[l]] for l, lv in enumerate(LEVELS)} for row in codes.tolist()]


def _same_out(got, ref, vocab, gt):
    assert got["best_threshold"] == ref["best_threshold"]
    assert got["micro_acc"] == ref["micro_acc"] and got["macro_acc"] == ref["macro_acc"] and got["per_class_acc"] == ref["per_class_acc"]
    assert got["final_pred_labels"] == _unpack(ref["final_pred_codes"], vocab)
    assert got["gt_labels"] == gt


def test_method_linear_equals_the_reference(ML, ops, dev, golden):
    """With the GOLDEN head loaded, under ==: evaluate_epoch, the list and the device form of inference_with_fine_tuned_image_encoder, the
    hit counts on all 1 001 thresholds, the chosen threshold, and both output dicts (micro, macro, per-class, merged predictions) at the
    searched and at a given threshold."""
    g = golden
    G, feats, img = _loaders(g, dev)
    head = torch.nn.Linear(128, 36)
    model = ML.ViTWIthExtraLayer(torch.nn.Identity(), head)
    model.load_state_dict({"new_linear_layer.weight": torch.from_numpy(g["head"]["weight"]), "new_linear_layer.bias": torch.from_numpy(g["head"]["bias"])})
    model.to(dev)
    label_map, idx_to_all = g["label_map"], g["idx_to_all_labels"]
    ev = ML.evaluate_epoch(model, img["seen_query"], dev, label_map)
    assert ev == g["final_evaluation"] and all(isinstance(v, float) for v in ev.values())
    sps = G.species_of()
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=g["k_list"]))
    splits = []
    original = _FeatureModel()
    keys = {s: _with_dna(img[s], feats[s][1], dev) for s in ("val_unseen_keys", "test_unseen_keys")}
    queries = {s: _with_dna(img[s], feats[s][1], dev) for s in ("seen_query", "unseen_query")}
    pb = ML.inference_with_original_image_encoder_and_dna_encoder(original, queries["seen_query"], queries["unseen_query"], keys["val_unseen_keys"],
                                                                  keys["test_unseen_keys"], dev)
    key_labels = G.labels_of(sps["val_unseen_keys"]) + G.labels_of(sps["test_unseen_keys"])
    for s, pred_b in zip(("seen_query", "unseen_query"), pb):
        conf, pred, gt = ML.inference_with_fine_tuned_image_encoder(model, img[s], label_map, idx_to_all, dev)
        assert np.array_equal(np.asarray([[label_map[x] for x in p["species"]] for p in pred]), g["idx"][s].astype(np.int64))
        assert pred[3] == {lv: [idx_to_all[int(i)][lv] for i in g["idx"][s][3]] for lv in LEVELS}
        assert gt == G.labels_of(sps[s])
        c = np.asarray(conf, dtype=np.float64)
        assert c.shape == (len(gt), 5) and np.abs(c - g["conf"][s].astype(np.float64)).max() < g["gap"] / 2
        dc, di, dgt = ML.classifier_topk(model, img[s], dev)
        assert dc.is_cuda and di.is_cuda and dc.dtype == torch.float32 and di.dtype == torch.int64 and dgt == gt
        assert np.array_equal(dc.cpu().numpy().astype(np.float64), c) and np.array_equal(di.cpu().numpy(), g["idx"][s].astype(np.int64))
        assert [p["species"] for p in pred_b] == [[key_labels[int(i)]["species"] for i in row] for row in g["idx_b"][s]]
        splits.append({"pred_labels_from_a": pred, "pred_confidence_from_a": conf, "pred_labels_from_b": pred_b, "gt_labels": gt})
    hits = ML.sweep_top1_hits(splits)
    assert hits.shape == (1001, 2) and np.array_equal(hits, g["hits"])
    assert ML.search_threshold_with_harmonic_mean(args, splits) == g["best"]
    for sp, name in zip(splits, ("seen", "unseen")):
        out = ML.get_final_pred_and_acc(args, sp["pred_labels_from_a"], sp["pred_confidence_from_a"], sp["pred_labels_from_b"], sp["gt_labels"],
                                        best_threshold=g["best"])
        _same_out(out, g["out"][name], g["vocab"], sp["gt_labels"])
    # end to end, loaders in: the searched threshold, then a given one
    so, uo = ML.method_2_inference_and_eval_for_seen_and_unseen(args, model, original, queries["seen_query"], queries["unseen_query"], keys["val_unseen_keys"],
                                                                keys["test_unseen_keys"], label_map, idx_to_all, dev)
    _same_out(so, g["out"]["seen"], g["vocab"], splits[0]["gt_labels"])
    _same_out(uo, g["out"]["unseen"], g["vocab"], splits[1]["gt_labels"])
    so, uo = ML.method_2_inference_and_eval_for_seen_and_unseen(args, model, original, queries["seen_query"], queries["unseen_query"], keys["val_unseen_keys"],
                                                                keys["test_unseen_keys"], label_map, idx_to_all, dev, searched_threshold=g["given_threshold"])
    _same_out(so, g["out_at"]["seen"], g["vocab"], splits[0]["gt_labels"])
    _same_out(uo, g["out_at"]["unseen"], g["vocab"], splits[1]["gt_labels"])
    # the device convention on tensors, merged indices instead of label lists
    logits = {s: ops.linear_f32_fwd(torch.from_numpy(feats[s][0]).to(dev), model.new_linear_layer.weight.detach(), model.new_linear_layer.bias.detach())
              for s in ("seen_query", "unseen_query")}
    kb = np.concatenate([feats["val_unseen_keys"][1], feats["test_unseen_keys"][1]])
    class_labels = [idx_to_all[i] for i in range(36)]
    so, uo = ML.classifier_seen_unseen_from_features(logits["seen_query"], logits["unseen_query"], class_labels, feats["seen_query"][0], feats["unseen_query"][0],
                                                     kb, key_labels, splits[0]["gt_labels"], splits[1]["gt_labels"], g["k_list"], with_predictions=False)
    assert so["best_threshold"] == g["best"] and so["micro_acc"] == g["out"]["seen"]["micro_acc"] and uo["macro_acc"] == g["out"]["unseen"]["macro_acc"]
    table = class_labels + key_labels
    assert [[table[int(i)]["species"] for i in row] for row in so["final_pred_labels"]] == [p["species"] for p in _unpack(g["out"]["seen"]["final_pred_codes"], g["vocab"])]


# --------------------------------------------------------------------------------------------------------- one fine-tuning step
def _encoder_and_oracle():
    from oracle import clibd_oracle as O
    from clibd_amd.model import create_vit
    from clibd_amd.simclr import SimCLRViT

    torch.manual_seed(3)
    om = O.VisionTransformer(img_size=224, patch=16, dim=384, depth=2, heads=6, num_classes=384)
    vit = create_vit("vit_small_patch16_224", num_classes=384, depth=2)
    vit.load_state_dict(om.state_dict(), strict=True)
    return O, om, vit, SimCLRViT(vit)


def test_one_fine_tuning_step_matches_oracle(ML, dev):
    """A two-block ViT-S-wide encoder (384, 6 heads) + head(384 -> 37) at b = 4 against the CPU oracle's ViT with the kernels' bf16 rounding
    points and torch's fp64 Linear + cross_entropy on top: construction, images and gates of
    tests/test_simclr_gpu.py::test_simclr_step_matches_oracle (gradients rel < 3e-2 and cosine > 0.999, the loss within 1e-3)."""
    from tests.test_simclr_gpu import _views

    O, om, vit, enc = _encoder_and_oracle()
    head = torch.nn.Linear(384, 37)
    images, _ = _views(torch.Generator().manual_seed(4))
    target = torch.tensor([0, 36, 5, 36])
    with O.precision("bf16"):
        fo = om(images)
        hw, hb = head.weight.detach().double().requires_grad_(True), head.bias.detach().double().requires_grad_(True)
        lo = F.cross_entropy(F.linear(fo.double(), hw, hb), target)
        ops_ = dict(om.named_parameters())
        grads = torch.autograd.grad(lo, list(ops_.values()) + [hw, hb])
        go = dict(zip(list(ops_) + ["new.weight", "new.bias"], grads))
    model = ML.ViTWIthExtraLayer(enc, head).to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    loss = ML.CrossEntropyLoss()(model(images.to(dev)), target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu().clone() for n, p in vit.named_parameters()}
    got["new.weight"], got["new.bias"] = head.weight.grad.detach().cpu(), head.bias.grad.detach().cpu()
    cos = lambda a, b: (a.double().flatten() @ b.double().flatten() / (a.double().norm() * b.double().norm() + 1e-30)).item()
    print(f"loss {loss.item():.6f} oracle {lo.item():.6f}")
    assert abs(loss.item() - lo.item()) < 1e-3, (loss.item(), lo.item())
    for n in ("new.weight", "new.bias", "head.weight", "blocks.0.attn.qkv.weight", "patch_embed.proj.weight", "pos_embed"):
        print(f"{n}: grad rel {rel_err(got[n], go[n]):.3e} cos {cos(got[n], go[n]):.6f}")
        assert rel_err(got[n], go[n]) < 3e-2 and cos(got[n], go[n]) > 0.999, (n, rel_err(got[n], go[n]), cos(got[n], go[n]))
    assert sorted(k for k in model.state_dict() if not k.startswith("vit.")) == ["new_linear_layer.bias", "new_linear_layer.weight"]


def test_strict_linear_probe_trains_only_the_head(ML, dev):
    from tests.test_simclr_gpu import _views

    _, _, vit, enc = _encoder_and_oracle()
    head = torch.nn.Linear(384, 37)
    model = ML.ViTWIthExtraLayer(enc, head, train_encoder=False).to(dev)
    images, _ = _views(torch.Generator().manual_seed(4))
    loss = ML.CrossEntropyLoss()(model(images.to(dev)), torch.tensor([0, 36, 5, 36], device=dev))
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in vit.parameters())
    assert head.weight.grad is not None and head.weight.grad.abs().sum().item() > 0 and head.bias.grad.abs().sum().item() > 0
    # build_image_classifier: a copy with its own tower, the head sized by the label map, the encoder frozen for the strict probe
    original = types.SimpleNamespace(image_encoder=enc)
    enc.tower()
    clf = ML.build_image_classifier(original, 37, train_encoder=False)
    assert clf.vit is not enc and clf.vit._tower is None and enc._tower is not None
    assert tuple(clf.new_linear_layer.weight.shape) == (37, 384) and clf.new_linear_layer.weight.is_cuda
    assert not any(p.requires_grad for p in clf.vit.parameters()) and all(p.requires_grad for p in clf.new_linear_layer.parameters())
    assert all(p.requires_grad for p in ML.build_image_classifier(original, 37).vit.parameters())


# ------------------------------------------------------------------------------------------------------------------- checkpoint
def test_last_pth_round_trip(ML, dev, golden, tmp_path):
    g = golden
    _, _, img = _loaders(g, dev)
    torch.manual_seed(9)
    model = ML.ViTWIthExtraLayer(torch.nn.Linear(128, 128), torch.nn.Linear(128, 36)).to(dev)
    args = types.SimpleNamespace(save_ckpt=True, model_config=types.SimpleNamespace(
        fine_tuning_set=types.SimpleNamespace(epochs=2, fine_tune_model_output_dir=str(tmp_path / "ft"))))
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    r = ML.train_image_classifier(args, model, img["train_seen"], img["seen_query"], None, dev, g["label_map"])
    assert not r["loaded"] and len(r["epoch_losses"]) == 2 and all(np.isfinite(r["epoch_losses"]))
    assert set(r["evaluation"][0]) == {"top1_accuracy", "top3_accuracy", "top5_accuracy"}
    sd = torch.load(r["last_ckpt_path"], map_location="cpu")
    assert r["last_ckpt_path"].endswith("last.pth")
    assert sorted(sd) == ["new_linear_layer.bias", "new_linear_layer.weight", "vit.bias", "vit.weight"]
    assert all(not v.is_cuda and v.untyped_storage().nbytes() == v.numel() * 4 for v in sd.values())
    assert all(not torch.equal(sd[k], before[k]) for k in sd)                       # the encoder trained too
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    # a second call finds last.pth: it loads it, freezes everything and does not train
    torch.manual_seed(10)
    fresh = ML.ViTWIthExtraLayer(torch.nn.Linear(128, 128), torch.nn.Linear(128, 36)).to(dev)
    r2 = ML.train_image_classifier(args, fresh, img["train_seen"], img["seen_query"], None, dev, g["label_map"])
    assert r2["loaded"] and r2["epoch_losses"] == []
    assert not any(p.requires_grad for p in fresh.parameters())
    for k, v in fresh.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    # and it travels to a plain torch module with the reference's layout
    class Ref(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.vit, self.new_linear_layer = torch.nn.Linear(128, 128), torch.nn.Linear(128, 36)

    Ref().load_state_dict(sd, strict=True)
