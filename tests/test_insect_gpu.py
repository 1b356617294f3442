"""GPU checks of the INSECT / BZSL workflow (clibd_amd.insect, include/clibd_hip_insect.h): the class means under `==` against the
row-order restatement of tests/insect_reference.py, the logits' top-k against torch's stable sort, the joint fine-tuning replayed from
the fixture's initial heads (tests/golden/insect_golden.pt), one joint step of real towers against the CPU oracle, the parameters the
classifiers share with the model, the checkpoints and CSV tables of the driver, and the four-loader eval phase."""
import functools
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import insect_reference as IR  # noqa: E402


@functools.lru_cache(maxsize=None)
def _gen():
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    spec = importlib.util.spec_from_file_location("make_insect_golden", ROOT / "tests" / "golden" / "make_insect_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _golden():
    return torch.load(ROOT / "tests" / "golden" / "insect_golden.pt", weights_only=False)


@pytest.fixture(scope="module")
def golden():
    return _golden()


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def I(dev):
    from clibd_amd import insect

    return insect


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ============================================================================================================== the class means
@functools.lru_cache(maxsize=None)
def _mean_case(name):
    """(x float32 [N, D], labels int32 [N], C); the reference is computed once per (case, order) by _mean_ref"""
    G = _gen()
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == "world":                                     # the fixture's world: both query splits, 36 classes
        x = np.concatenate([G.MLG.synth("seen_query")[0], G.MLG.synth("unseen_query")[0]])
        sp = G.MLG.species_of()
        labels = (np.concatenate([sp["seen_query"], sp["unseen_query"]]) % 36).astype(np.int32)
        return x, labels, 36
    N, C, D = {"smallest": (1, 1, 1), "odd": (7, 3, 5), "long": (1000, 5, 768), "strided": (257, 40, 130), "threshold": (8193, 3, 3)}[name]
    x = (rs.randn(N, D) * np.exp(rs.randn(N, 1))).astype(np.float32)
    labels = rs.randint(0, C, N).astype(np.int32)
    if name == "threshold":                                 # 4 096 rows: the longest list sorted in LDS; 4 097: the ordered rescan; one empty class
        labels = rs.permutation(np.repeat(np.array([0, 1], dtype=np.int32), [4096, 4097]))
    if name == "long":                                      # one class holds 900 rows
        labels[rs.permutation(N)[:900]] = 2
        assert (labels == 2).sum() >= 900
    return x, labels, C


@functools.lru_cache(maxsize=None)
def _mean_ref(name, order):
    x, labels, C = _mean_case(name)
    if order == "sorted":
        perm = np.argsort(labels, kind="stable")
        x, labels = x[perm], labels[perm]
    mean, count, error = IR.class_mean(x, labels, C)
    assert error == 0
    return x, labels, C, mean, count


@pytest.mark.parametrize("name", ["smallest", "odd", "world", "long", "strided", "threshold"])
def test_class_mean_equals_the_row_order_restatement(ops, dev, name):
    for order in ("sorted", "shuffled"):
        x, labels, C, ref, ref_count = _mean_ref(name, order)
        N, D = x.shape
        if name == "strided":                               # ld_x > D
            xd = torch.zeros((N, D + 6), dtype=torch.float32, device=dev)[:, :D]
            xd.copy_(torch.from_numpy(x))
            assert xd.stride(0) == D + 6
        else:
            xd = torch.from_numpy(x).to(dev)
        ld = torch.from_numpy(labels).to(dev)
        for transposed in (False, True):
            want = ref.T if transposed else ref
            mean, count, error = ops.class_mean(xd, ld, C, transposed=transposed)
            assert np.array_equal(bits(mean), bits(want)), (name, order, transposed)
            assert np.array_equal(count.cpu().numpy(), ref_count) and int(error.item()) == 0
            rows, cols = want.shape                         # a padded leading dimension: the padding is not written
            buf = torch.full((rows, cols + 3), 7.0, dtype=torch.float32, device=dev)
            ops.class_mean(xd, ld, C, transposed=transposed, out=buf[:, :cols])
            assert np.array_equal(bits(buf[:, :cols]), bits(want)), (name, order, transposed, "padded")
            assert bool((buf[:, cols:] == 7.0).all())


def test_class_mean_empty_class_bad_label_and_repeat(ops, dev):
    x, labels, C, _, _ = _mean_ref("odd", "shuffled")
    xd = torch.from_numpy(x).to(dev)
    # an empty class: a zero row and count 0
    mean, count, error = ops.class_mean(xd, torch.from_numpy(labels).to(dev), C + 2)
    ref, ref_count, _ = IR.class_mean(x, labels, C + 2)
    assert np.array_equal(bits(mean), bits(ref)) and count.cpu().tolist() == ref_count.tolist()
    assert count.cpu().tolist()[-2:] == [0, 0] and not mean[-2:].any().item() and int(error.item()) == 0
    # a label outside [0, C) sets the error bit and changes nothing else
    bad = labels.copy()
    bad[2], bad[5] = -1, C
    ref, ref_count, ref_error = IR.class_mean(x, bad, C)
    mean, count, error = ops.class_mean(xd, torch.from_numpy(bad).to(dev), C)
    assert ref_error == 1 and int(error.item()) == 1
    assert np.array_equal(bits(mean), bits(ref)) and count.cpu().tolist() == ref_count.tolist()
    keep = np.ones(len(bad), bool)
    keep[[2, 5]] = False
    assert np.array_equal(bits(ref), bits(IR.class_mean(x[keep], bad[keep], C)[0]))
    # two calls are bit-identical (the long chain, the atomic fill in front of it)
    x, labels, C, ref, _ = _mean_ref("long", "shuffled")
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    a = ops.class_mean(xd, ld, C)[0].clone()
    b = ops.class_mean(xd, ld, C)[0]
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(ref))


def test_class_embeddings_reproduce_the_golden_table_and_csv(I, dev, golden, tmp_path):
    G = _gen()
    feats, labels = G.proto_world()
    p = golden["proto"]
    table = I.class_embeddings(feats, labels)
    assert table.dtype == np.float32 and np.array_equal(bits(table), bits(p["class_embed"]))
    assert IR.savetxt_text(table) == p["text"]
    # the device form on dense labels, and the two files
    dense = np.unique(labels, return_inverse=True)[1]
    mean, count = I.class_mean_embeddings(torch.from_numpy(feats).to(dev), torch.from_numpy(dense).to(dev))
    assert np.array_equal(bits(mean), bits(p["class_embed"].T)) and count.cpu().tolist() == p["sizes"]
    with pytest.raises(ValueError, match="outside"):
        I.class_mean_embeddings(torch.from_numpy(feats).to(dev), dense, num_classes=len(p["sizes"]) - 1)
    img = np.random.RandomState(3).randn(len(labels), 8)
    d = {"encoded_dna_feature": torch.from_numpy(feats).to(dev), "encoded_image_feature": img}
    I.save_bzsl_embeddings(tmp_path / "dna.csv", tmp_path / "image.csv", d, labels)
    assert (tmp_path / "dna.csv").read_text() == p["text"]
    assert (tmp_path / "image.csv").read_text() == IR.savetxt_text(img.astype(np.float32).T)


# ============================================================================================================ the logits' top-k
@pytest.mark.parametrize("B,C,k", [(1, 1, 1), (3, 5, 5), (33, 36, 5), (16, 916, 8), (7, 1213, 8)])
def test_logits_topk_equals_the_stable_sort(ops, dev, B, C, k):
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = torch.round(torch.randn(B, C, generator=g) * 4) / 2                 # multiples of 0.5: many ties
    logits[torch.rand(B, C, generator=g) < 0.1] = -float("inf")
    if B > 2:
        logits[1] = -float("inf")                                               # a whole row of -inf: the first k indices
        logits[2] = 1.25                                                        # a whole row of one value
    buf = torch.zeros((B, C + 3), dtype=torch.float32, device=dev)              # a strided ld
    view = buf[:, :C]
    view.copy_(logits)
    for t in (view, logits.to(dev)):
        val, idx = ops.logits_topk(t, k)
        rv, ri = IR.logits_topk(logits, k)
        assert torch.equal(idx.cpu(), ri) and np.array_equal(bits(val), bits(rv)), (B, C, k)
    assert idx.dtype == torch.int64 and val.dtype == torch.float32 and tuple(idx.shape) == (B, k)


def test_logits_topk_follows_the_logits_where_softmax_topk_cannot(ops, dev):
    row = torch.tensor([[0.0, -200.0, -150.0, -120.0, -110.0, -300.0, -250.0, -105.0]])
    val, idx = ops.logits_topk(row.to(dev), 5)
    assert idx.cpu().tolist() == [[0, 7, 4, 3, 2]] == IR.logits_topk(row, 5)[1].tolist()
    assert val.cpu().tolist() == [[0.0, -105.0, -110.0, -120.0, -150.0]]
    conf, sidx = ops.softmax_topk(row.to(dev), 5)
    # the confidences underflow to one value: what softmax_topk reports no longer tells the four classes apart, and a ranking of the
    # fp32 confidences (torch.topk(F.softmax(row)), what a confidence-ranked evaluation sees) falls back to the index order.  The kernel
    # itself selects on the logits before it forms the confidences, so the indices it returns beside them still follow the logits.
    assert val.cpu()[0].unique().numel() == 5 and conf.cpu()[0, 1:].unique().numel() == 1
    by_conf = torch.sort(F.softmax(row, dim=-1), dim=1, descending=True, stable=True)[1][:, :5]
    assert by_conf.tolist() == [[0, 1, 2, 3, 4]] != idx.cpu().tolist()
    assert sidx.cpu().tolist() == idx.cpu().tolist()
    with pytest.raises(RuntimeError, match="out of range"):
        ops.logits_topk(torch.zeros(2, 4, device=dev), 5)
    with pytest.raises(ValueError):
        ops.logits_topk(torch.zeros(2, 16, device=dev), 9)


# ================================================================================================== the joint fine-tuning replay
def _classifiers(I, heads, dev):
    out = []
    for m in ("image", "dna"):
        lin = torch.nn.Linear(128, 36)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(heads[m]["weight"]))
            lin.bias.copy_(torch.from_numpy(heads[m]["bias"]))
        out.append(I.EncoderWithExtraLayer(torch.nn.Identity(), lin).to(dev))
    return out


def test_joint_fine_tuning_follows_the_reference(I, dev, golden):
    """fine_tuning_epoch_image_and_dna with identity encoders on the golden batches, from the recorded initial heads, one FusedAdamW at
    the generator's lr: every step's summed loss within 2e-4 |ref| + 2e-3 of the reference's (test_method_linear_gpu.py's per-loss
    gate, once per summand); then evaluate_epoch on both modalities."""
    from clibd_amd.optim import FusedAdamW

    g, G = golden, _gen()
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    train = G.joint_loader("train_seen", g["batch"], to_dev)
    evalq = G.joint_loader("seen_query", g["query_batch"], to_dev, g["eval_redraw"])
    ic, dc = _classifiers(I, g["head0"], dev)
    opt = FusedAdamW(I.combined_parameters(ic, dc), lr=g["lr"])
    steps, epoch_losses = [], []
    for epoch in range(g["epochs"]):
        epoch_losses.append(I.fine_tuning_epoch_image_and_dna(None, ic, dc, train, opt, I.CrossEntropyLoss(), g["species"], epoch, dev, step_losses=steps))
    got = torch.stack(steps).cpu().double().numpy()
    ref = g["step_losses"]
    diff = np.abs(got - ref)
    print(f"{len(ref)} joint steps: loss {got[0]:.5f} -> {got[-1]:.5f} (reference {ref[0]:.5f} -> {ref[-1]:.5f}), max |loss - reference| {diff.max():.3e}")
    assert got.shape == ref.shape and (diff <= 2e-4 * np.abs(ref) + 2e-3).all(), diff.max()
    assert got[-1] < 0.1 * got[0]
    assert np.allclose(epoch_losses, g["epoch_losses"], rtol=0, atol=2e-4 * ref.max() + 2e-3)
    for m, clf in (("image", ic), ("dna", dc)):
        ev = I.evaluate_epoch(clf, evalq, dev, g["species"], modality=m)
        assert all(isinstance(v, np.float64) for v in ev.values()) and not clf.training
        assert {k: float(v) for k, v in ev.items()} == g["evaluation"][m], (m, ev)
    # the golden's trained heads: the dicts and the indices themselves
    ic, dc = _classifiers(I, g["head"], dev)
    for m, clf in (("image", ic), ("dna", dc)):
        ev = I.evaluate_epoch(clf, evalq, dev, g["species"], k_values=g["k_values"], modality=m)
        assert {k: float(v) for k, v in ev.items()} == g["evaluation"][m], (m, ev)
        idx, target = I.predict_topk(clf.eval(), evalq, dev, g["species"], 5, modality=m)
        assert np.array_equal(idx.cpu().numpy(), g["argsort"][m].astype(np.int64)), m
        assert target.tolist() == [g["species"].index(f"s{int(s)}") for s in G.MLG.species_of()["seen_query"]]
    # the single-modality epoch with a scheduler steps both
    from torch.optim.lr_scheduler import OneCycleLR

    ic, _ = _classifiers(I, g["head0"], dev)
    opt = FusedAdamW(ic.parameters(), lr=g["lr"])
    sched = OneCycleLR(opt, max_lr=g["lr"], total_steps=len(train))
    first = []
    loss = I.fine_tuning_epoch(None, ic, train, opt, I.CrossEntropyLoss(), g["species"], 0, dev, modality="image", scheduler=sched, step_losses=first)
    assert np.isfinite(loss) and abs(float(first[0]) - g["step_summands"][0, 0]) <= 2e-4 * g["step_summands"][0, 0] + 1e-3
    assert sched.last_epoch == len(train)


# ============================================================================================== one joint step of real towers
def _real_towers(dev, full):
    from oracle import clibd_oracle as O
    from clibd_amd.model import CLIBDImageEncoder, VisionTransformer
    from tests.test_model_gpu import hip_dna, load, oracle_models

    gd = load("dna_tiny_golden.pt")                          # a two-layer BERT of hidden 128
    od, md = oracle_models()[0](gd), hip_dna(gd, dev)
    torch.manual_seed(21)
    oi = O.ImageEncoder(O.VisionTransformer(img_size=224, patch=16, dim=384, depth=2, heads=6, num_classes=10), r=4, num_classes=128)
    with torch.no_grad():
        for _, p in oi.named_parameters():
            if p.dim() == 2 and not bool(p.any()):           # the LoRA B matrices start at zero: give the adapters a gradient
                p.normal_(std=0.02)
    mi = CLIBDImageEncoder(VisionTransformer(embed_dim=384, depth=2, num_heads=6, num_classes=10), r=4, num_classes=128)
    mi.load_state_dict(oi.state_dict(), strict=True)
    mi = mi.to(dev).eval()
    oi = oi.eval()
    if full:
        for mod in (oi, od, mi, md):
            for p in mod.parameters():
                p.requires_grad_(True)
    return O, oi, od, mi, md, gd["ids"]


@pytest.mark.parametrize("full", [False, True], ids=["lora", "disable_lora"])
def test_one_joint_step_matches_oracle(I, dev, full):
    """A two-block ViT-S-wide image encoder (384, 6 heads) and a two-layer BERT (hidden 128) under two 37-way heads at b = 4 against the
    CPU oracle with the kernels' bf16 rounding points and torch's fp64 Linear + cross_entropy on top — the gates of
    test_method_linear_gpu.py::test_one_fine_tuning_step_matches_oracle: gradients rel < 3e-2 and cosine > 0.999 for every trainable
    tensor of both towers and both heads, the summed loss within 2e-3."""
    from tests.test_model_gpu import assert_grads, cos, rel

    O, oi, od, mi, md, ids = _real_towers(dev, full)
    torch.manual_seed(22)
    hi, hd = torch.nn.Linear(128, 37), torch.nn.Linear(128, 37)
    images = torch.rand(4, 3, 224, 224, generator=torch.Generator().manual_seed(23))
    target = torch.tensor([0, 36, 5, 36])
    with O.precision("bf16"):
        heads = [t.detach().double().requires_grad_(True) for t in (hi.weight, hi.bias, hd.weight, hd.bias)]
        lo = (F.cross_entropy(F.linear(oi(images).double(), heads[0], heads[1]), target)
              + F.cross_entropy(F.linear(od(ids).double(), heads[2], heads[3]), target))
        named = [(f"image.{n}", p) for n, p in oi.named_parameters() if p.requires_grad] + [(f"dna.{n}", p) for n, p in od.named_parameters() if p.requires_grad]
        grads = torch.autograd.grad(lo, [p for _, p in named] + heads, allow_unused=True)
        go = {n: (torch.zeros_like(p) if g is None else g.detach()) for (n, p), g in zip(named, grads)}
        gh = [g.detach() for g in grads[len(named):]]
    ic, dc = I.EncoderWithExtraLayer(mi, hi).to(dev).eval(), I.EncoderWithExtraLayer(md, hd).to(dev).eval()
    crit = I.CrossEntropyLoss()
    loss = crit(ic(images.to(dev)), target.to(dev)) + crit(dc(ids.to(dev)), target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    got = {}
    for prefix, mod in (("image", mi), ("dna", md)):
        for n, p in mod.named_parameters():
            if p.requires_grad:
                got[f"{prefix}.{n}"] = (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu()
    print(f"joint loss {loss.item():.6f} oracle {lo.item():.6f} ({len(got)} tower tensors)")
    assert abs(loss.item() - lo.item()) < 2e-3, (loss.item(), lo.item())
    assert len(got) > (60 if full else 10)
    if full:
        assert_grads(got, go, rel_tol=3e-2, cos_tol=0.999, what="joint step, disable_lora", zero_tol=2e-6, zero_rel=1e-4)
    else:
        assert_grads(got, go, rel_tol=3e-2, cos_tol=0.999, what="joint step, LoRA")
    worst = (0.0, 1.0)
    for name, p, r in (("image head weight", hi.weight, gh[0]), ("image head bias", hi.bias, gh[1]), ("dna head weight", hd.weight, gh[2]),
                       ("dna head bias", hd.bias, gh[3])):
        e, c = rel(p.grad.cpu(), r), cos(p.grad.cpu(), r)
        worst = (max(worst[0], e), min(worst[1], c))
        assert e < 3e-2 and c > 0.999, (name, e, c)
    tower_rel = max(rel(got[n], go[n]) for n in go if go[n].abs().max() > 1e-4 * max(float(v.abs().max()) for v in go.values()))
    print(f"heads: worst rel {worst[0]:.3e}, worst cosine {worst[1]:.6f}; towers: worst rel {tower_rel:.3e}")


# ================================================================================== shared parameters, checkpoints, the driver
def _tiny_model_and_loader(dev):
    from clibd_amd.model.simple_clip import SimpleCLIP
    from tests.test_model_gpu import hip_dna, hip_image, load

    gd, gi = load("dna_tiny_golden.pt"), load("image_tiny_golden.pt")
    model = SimpleCLIP(hip_image(gi, dev), hip_dna(gd, dev), None).to(dev)
    img = gi["image_u8"].float() / 255.0
    species = [["a", "b", "c"], ["c", "a", "a"]]
    loader = []
    for b, sp in enumerate(species):
        labels = {"order": ["o"] * 3, "family": ["f"] * 3, "genus": ["g" + s for s in sp], "species": sp}
        loader.append(([f"id{b}{i}" for i in range(3)], img.flip(0) if b else img, gd["ids"][b:b + 3], None, None, None, labels))
    return model, loader, np.array([4, 9, 2, 2, 4, 4])


def test_driver_trains_the_models_own_towers_and_writes_checkpoints_and_tables(I, dev, golden, tmp_path):
    from clibd_amd import eval as E

    model, loader, labels = _tiny_model_and_loader(dev)
    args = types.SimpleNamespace(save_ckpt=True, model_config=types.SimpleNamespace(
        output_dim=128, evaluation_period=1, fine_tuning_set=types.SimpleNamespace(epochs=2)))
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    r = I.supervised_fine_tune(args, model, loader, loader, loader, labels, dev, out_dir=str(tmp_path), unique_species_for_seen=["a", "b", "c"])
    ic, dc = r["image_classifier"], r["dna_classifier"]
    assert ic.encoder is model.image_encoder and dc.encoder is model.dna_encoder                       # wrapped, not copied
    assert len(r["epoch_losses"]) == 2 and all(np.isfinite(r["epoch_losses"])) and [e for e, _, _ in r["evaluation"]] == [0, 1]
    assert set(r["evaluation"][0][1]) == set(r["evaluation"][0][2]) == {"top1_accuracy", "top3_accuracy", "top5_accuracy"}
    after = {n: p.detach().cpu() for n, p in model.named_parameters()}
    moved = {n for n in before if not torch.equal(before[n], after[n])}
    assert moved <= trainable                                                                          # the frozen base weights stay
    for tower in ("image_encoder", "dna_encoder"):
        mine = {n for n in trainable if n.startswith(tower + ".")}
        assert mine and mine <= moved, (tower, sorted(mine - moved))                                   # a step moves original_model's towers
    # state-dict keys: the reference's, for the wrapper and the head
    ref_keys = golden["ref_state_dict_keys"]
    lin = I.EncoderWithExtraLayer(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2))
    assert list(lin.state_dict()) == ref_keys
    for clf, enc in ((ic, model.image_encoder), (dc, model.dna_encoder)):
        assert list(clf.state_dict()) == ["encoder." + k for k in enc.state_dict()] + [k for k in ref_keys if k.startswith("new_linear_layer.")]
    # image_last.ckpt / dna_last.ckpt round-trip
    assert r["image_last_ckpt_path"].endswith("image_last.ckpt") and r["dna_last_ckpt_path"].endswith("dna_last.ckpt")
    for clf, path in ((ic, r["image_last_ckpt_path"]), (dc, r["dna_last_ckpt_path"])):
        sd = torch.load(path, map_location="cpu")
        assert list(sd) == list(clf.state_dict()) and all(not v.is_cuda for v in sd.values())
        for k, v in clf.state_dict().items():
            assert torch.equal(v.cpu(), sd[k]), k
        clf.load_state_dict(sd, strict=True)
    # the two tables: the prototypes of the fine-tuned DNA encoder's features, the image features transposed
    d = E.get_features_and_label(loader, model, dev, as_numpy=True)
    assert open(r["dna_embed_path"]).read() == IR.savetxt_text(IR.class_embeddings(d["encoded_dna_feature"], labels))
    assert open(r["image_embed_path"]).read() == IR.savetxt_text(d["encoded_image_feature"].astype(np.float32).T)
    assert np.loadtxt(r["dna_embed_path"], delimiter=",").shape == (128, 3) and np.loadtxt(r["image_embed_path"], delimiter=",").shape == (128, 6)


# ========================================================================================================= the INSECT eval phase
class _FeatureModel(torch.nn.Module):
    """a tiny 'model': a loader's image batch holds image features, its dna batch DNA features"""

    image_encoder = dna_encoder = True
    language_encoder = None

    def forward(self, image, dna, language):
        return image, dna, None


def test_insect_eval_phase_equals_the_host_concatenated_dicts(I, dev):
    from clibd_amd import eval as E

    G = _gen()
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    loaders = [G.joint_loader(s, 64, to_dev) for s in ("train_seen", "val_unseen_keys", "seen_query", "unseen_query")]
    model = _FeatureModel()
    acc, pred = I.eval_phase(model, dev, *loaders, [1, 3, 5])
    host = [E.get_features_and_label(l, model, dev, as_numpy=True) for l in loaders]
    keys = I.construct_key_dict(host)
    assert keys["encoded_image_feature"].shape == (108 + 150 + 200 + 150, 128) and len(keys["label_list"]) == 608
    acc_ref, _, pred_ref = E.inference_and_print_result(keys, host[2], host[3], k_list=[1, 3, 5])
    assert acc == acc_ref and pred == pred_ref
    assert set(acc["encoded_image_feature"]["encoded_dna_feature"]) == {"seen", "unseen"}
    value = I.overall_acc(acc)
    per = acc["encoded_image_feature"]["encoded_image_feature"]
    assert value == (per["seen"]["micro_acc"][1]["species"] + per["unseen"]["micro_acc"][1]["species"]) / 2 and 0.0 < value <= 1.0
