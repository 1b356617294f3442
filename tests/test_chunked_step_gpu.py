"""GPU checks of the chunked contrastive step (clibd_amd.chunked, Trainer(chunk_size=...), SimCLR(chunk_size=...)).

Fixtures: the b = 8 reference step of tests/golden/step_tiny_golden.pt (tiny towers), the two-block ViT-S-wide tower of tests/test_simclr_gpu.py, and,
where a check is on bits (torch.equal), the b = 8 LoRA step of tests/test_deterministic_mode_gpu.py: the plain step's LoRA gradients do not repeat bit for
bit on the tiny towers even in deterministic mode (two plain steps differ in 2-4 thousand of 41280 bucket words by 1e-6 relative), so nothing can equal them.
Gates, none of them new:
  * cached embeddings against the plain step's forward 1e-6 (unit-norm rows; tests/test_metric_config_gpu.py's gate for row independence);
  * loss against the plain step's 1e-5; gradients against the plain step's over the whole vector: relative difference < 2e-3 and cosine > 0.99999
    (test_b2048_backward_is_the_sum_of_chunk_backwards);
  * against the bf16 oracle and the reference's fp32 goldens: the numbers of tests/test_model_gpu.py::test_full_step_matches_reference;
  * train mode against the oracle evaluated chunk by chunk with the chunks' dropout bases: the oracle-bf16 gates of that same test (an end-to-end
    contrastive gradient against the bf16 oracle: the comparison those numbers were set for), masks as in test_bert_train_mode_dropout_matches_oracle_masks;
  * optimizer.grad_norm against the fp64 norm of the accumulated bucket: tests/optim_reference.norm_gate.
Every figure is printed before it is asserted.  Measured on an MI355X: see DESIGN §3.19.  There is no run on more than one GPU: the two-rank case shares
the GPU over gloo."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests.test_model_gpu import assert_grads, cos, hip_dna, hip_image, hip_text, load, oracle_models, rel  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
_cache = {}


def goldens():
    if "g" not in _cache:
        _cache["g"] = tuple(load(n) for n in ("step_tiny_golden.pt", "dna_tiny_golden.pt", "text_tiny_golden.pt", "image_tiny_golden.pt"))
    return _cache["g"]


def build(tag, dev, train=False):
    from clibd_amd.model import SimpleCLIP

    gs, gd, gt, gi = goldens()
    model = SimpleCLIP(hip_image(gi, dev), hip_dna(gd, dev), hip_text(gt, dev) if tag == "idt" else None).to(dev)
    with torch.no_grad():
        model.logit_scale.copy_(gs["logit_scale"])
    return model.train(train)


def batch(tag, dev, rows=slice(None)):
    gs = goldens()[0]
    text = {k: v[rows].to(dev) for k, v in gs["text"].items()} if tag == "idt" else None
    return (gs["image_u8"][rows].float() / 255.0).to(dev), gs["dna"][rows].to(dev), text, gs["labels"][rows].to(dev)


def named_grads(model, divide=1.0):
    return {n: (torch.zeros_like(p) if p.grad is None else p.grad / divide).detach().cpu() for n, p in model.named_parameters() if p.requires_grad}


def whole(d, keys):
    return torch.cat([d[n].flatten() for n in keys])


def plain_step(tag, dev):
    """the plain Trainer.step on the fixture, eval mode: (loss, named gradients, embeddings of the step's own forward).  Computed once per tag."""
    if ("plain", tag) not in _cache:
        from clibd_amd.train import Trainer

        model = build(tag, dev)
        img, dna, text, labels = batch(tag, dev)
        emb = [None if e is None else e.detach().clone() for e in model(img, dna, text)[:3]]       # with grad enabled: the saving forward, as in the step
        tr = Trainer(model, lr=1e-3)
        loss = tr.step(img, dna, text, labels)
        _cache[("plain", tag)] = (float(loss), named_grads(model), emb, tr.optimizer.flat_g.clone())
    return _cache[("plain", tag)]


def oracle_step(tag):
    """the bf16 oracle's loss, gradients and embeddings on the fixture.  Computed once per tag."""
    if ("oracle", tag) not in _cache:
        from oracle import clibd_oracle as O

        gs, gd, gt, gi = goldens()
        build_dna, build_text, build_image = oracle_models()
        om = O.SimpleCLIP(build_image(gi), build_dna(gd), build_text(gt))
        with torch.no_grad():
            om.logit_scale.copy_(gs["logit_scale"])
        with O.precision("bf16"):
            oi, od, ot, osc, _ = om(gs["image_u8"].float() / 255.0, gs["dna"], gs["text"])
            lo = O.contrastive_loss([oi, od, ot if tag == "idt" else None], gs["labels"], osc)
            ps = [(n, p) for n, p in om.named_parameters() if p.requires_grad]
            go = {n: (torch.zeros_like(p) if g is None else g) for (n, p), g in zip(ps, torch.autograd.grad(lo, [p for _, p in ps], allow_unused=True))}
        _cache[("oracle", tag)] = (float(lo.detach()), go, [oi.detach(), od.detach(), ot.detach()])
    return _cache[("oracle", tag)]


def against_plain(got, want, what):
    """the project's gates for `a backward is the sum of its chunk backwards`, over the whole gradient vector"""
    keys = sorted(want)
    assert sorted(got) == keys
    a, e = whole(got, keys), whole(want, keys)
    r, c = rel(a, e), cos(a, e)
    print(f"{what}: gradient against the plain step's, whole vector: rel {r:.3e}, cosine {c:.8f}")
    assert r < 2e-3 and c > 0.99999, (what, r, c)
    return r, c


# ---- 1. exactness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [3, 4, 2])
@pytest.mark.parametrize("tag", ["id", "idt"])
def test_chunked_step_matches_plain_step_and_reference(dev, tag, chunk):
    from clibd_amd.train import Trainer

    gs = goldens()[0]
    loss_p, grads_p, emb_p, _ = plain_step(tag, dev)
    lo, go, emb_o = oracle_step(tag)
    model = build(tag, dev)
    tr = Trainer(model, lr=1e-3, chunk_size=chunk)
    with torch.no_grad():
        emb_ng = [None if e is None else e.clone() for e in model(*batch(tag, dev)[:3])[:3]]
    loss = float(tr.step(*batch(tag, dev)))
    got = named_grads(model)
    torch.cuda.synchronize()
    d_emb = max(float((c - e).abs().max()) for c, e in zip(tr.cached_embeddings, emb_p) if c is not None)
    d_ng = max(float((c - e).abs().max()) for c, e in zip(tr.cached_embeddings, emb_ng) if c is not None)
    print(f"{tag} chunk_size={chunk}: cached embeddings against the plain step's forward {d_emb:.3e} (against the plain no-grad forward {d_ng:.3e}); "
          f"loss {loss:.7f}, plain {loss_p:.7f} (off by {abs(loss - loss_p):.2e}), oracle {lo:.7f}, reference {float(gs[f'loss_{tag}']):.7f}; "
          f"replay_mismatch {int(tr.replay_mismatch)}; step_count {tr.optimizer.step_count}")
    assert [c is None for c in tr.cached_embeddings] == [False, False, tag == "id"] and all(c.shape == (8, 128) and c.dtype == F32 for c in tr.cached_embeddings if c is not None)
    assert d_emb <= 1e-6
    assert abs(loss - loss_p) <= 1e-5
    assert int(tr.replay_mismatch) == 0 and tr.optimizer.step_count == 1
    against_plain(got, grads_p, f"{tag} chunk_size={chunk}")
    # the bf16 oracle: test_full_step_matches_reference's numbers
    keys = sorted(got)
    assert set(keys) <= set(go) and all(n.startswith("language_encoder.") for n in set(go) - set(keys))
    for c, r in zip(tr.cached_embeddings, emb_o):
        if c is not None:
            assert (c.cpu() - r).abs().max().item() < 1e-3
    assert abs(loss - lo) < 1e-3
    assert_grads(got, {n: go[n] for n in keys}, rel_tol=0.2, cos_tol=0.98, what="chunked step vs oracle-bf16")
    a, e = whole(got, keys), whole(go, keys)
    print(f"{tag} chunk_size={chunk}: against the bf16 oracle, whole vector: rel {rel(a, e):.3e}, cosine {cos(a, e):.6f}")
    assert rel(a, e) < 0.08 and cos(a, e) > 0.997
    # the reference's fp32 goldens
    for c, r in zip(tr.cached_embeddings, gs[f"features_{tag}"]):
        if c is not None:
            assert (c.cpu() - r).abs().max().item() < 5e-3
    assert abs(loss - float(gs[f"loss_{tag}"])) < 2e-2
    gr = gs[f"grads_{tag}"]
    assert_grads(got, {n: gr[n] for n in keys}, rel_tol=0.25, cos_tol=0.97, what="chunked step vs reference fp32")
    e = whole(gr, keys)
    print(f"{tag} chunk_size={chunk}: against the reference's fp32 goldens, whole vector: rel {rel(a, e):.3e}, cosine {cos(a, e):.6f}")
    assert rel(a, e) < 0.1 and cos(a, e) > 0.995


# ---- 2. replay ---------------------------------------------------------------------------------------------------------------------------------
def _train_step(dev, chunk, seed=5, **kw):
    from clibd_amd.train import Trainer

    model = build("id", dev, train=True)          # DNA tower: HF BERT dropout p = 0.1 on; the ViT has none
    tr = Trainer(model, lr=1e-3, deterministic=True, chunk_size=chunk, **kw)
    torch.manual_seed(seed)
    loss = tr.step(*batch("id", dev))
    torch.cuda.synchronize()
    return model, tr, loss, torch.get_rng_state()


def det_step(dev, chunk, run=0, **kw):
    """One seeded train-mode step in deterministic mode on the fixture of tests/test_deterministic_mode_gpu.py (ViT-B + BarcodeBERT, LoRA r = 4,
    b = 8: the shapes on which the plain step is known to repeat bit for bit).  Results are kept per (chunk, run, settings); `run` asks for another,
    independent execution of the same step."""
    key = ("det", chunk, run, tuple(sorted(kw.items())))
    if key not in _cache:
        from test_deterministic_mode_gpu import _lora_model

        from clibd_amd.data import synthetic_batch
        from clibd_amd.train import Trainer

        bt = synthetic_batch(8, dev, seed=3, rank=0, with_text=False)
        model = _lora_model(dev, text=False)
        model.train(True)
        tr = Trainer(model, lr=1e-4, deterministic=True, chunk_size=chunk, **kw)
        torch.manual_seed(123)
        loss = tr.step(bt["image"], bt["dna"], bt["text"], bt["labels"])
        torch.cuda.synchronize()
        o = tr.optimizer
        _cache[key] = dict(loss=loss.clone(), g=o.flat_g.clone(), p=o.flat_p.clone(), rng=torch.get_rng_state(), step_count=o.step_count,
                           mismatch=None if tr.replay_mismatch is None else int(tr.replay_mismatch), grad_norm=o.grad_norm.item(),
                           coef=o._record.view(F32)[1].item(), steps_done=tr._steps_done)
    return _cache[key]


def test_one_chunk_two_passes_is_the_plain_step_bit_for_bit(dev):
    """chunk_size = b: the same base, the same local rows, the same order of launches behind the loss"""
    p, c = det_step(dev, None), det_step(dev, 8)
    diff = int((p["g"] != c["g"]).sum())
    print(f"chunk_size = b: loss {float(c['loss']):.9g} (plain {float(p['loss']):.9g}); bucket elements that differ {diff} of {p['g'].numel()}; "
          f"replay_mismatch {c['mismatch']}")
    assert torch.equal(p["loss"], c["loss"]) and torch.equal(p["g"], c["g"]) and float(p["g"].abs().max()) > 0
    assert torch.equal(p["rng"], c["rng"]) and c["mismatch"] == 0 and p["mismatch"] is None
    assert torch.equal(p["p"], c["p"]) and p["step_count"] == c["step_count"] == 1
    e = det_step(dev, 16)                           # chunk_size > b: one chunk as well
    assert torch.equal(e["g"], p["g"]) and torch.equal(e["rng"], p["rng"])


def test_ragged_chunks_replay_their_own_dropout_masks_and_match_the_oracle(dev):
    from oracle import clibd_oracle as O
    import torch.nn.functional as Fn

    model, tr, loss, _ = _train_step(dev, 3, seed=5)
    got = named_grads(model)
    # the documented order of draws: pass 1, chunk after chunk, one base per tower with dropout (here the DNA tower only)
    torch.manual_seed(5)
    bases = [int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) for _ in range(3)]
    print(f"chunk_size=3, train mode: replay_mismatch {int(tr.replay_mismatch)}; dropout bases {bases}; loss {float(loss):.7f}")
    assert int(tr.replay_mismatch) == 0
    assert len(set(bases)) == 3
    gs, gd, gt, gi = goldens()
    build_dna, _, build_image = oracle_models()
    om = O.SimpleCLIP(build_image(gi), build_dna(gd), None)
    with torch.no_grad():
        om.logit_scale.copy_(gs["logit_scale"])
    img = gs["image_u8"].float() / 255.0
    with O.precision("bf16"):
        oi = Fn.normalize(om.image_encoder(img).float(), p=2, dim=-1)
        od = []
        for (lo_, hi_), base in zip(((0, 3), (3, 6), (6, 8)), bases):
            with O.dropout(0.1, 0.1, base):              # the chunk's base, element indices local to the chunk
                od.append(Fn.normalize(om.dna_encoder(gs["dna"][lo_:hi_]).float(), p=2, dim=-1))
        od = torch.cat(od)
        lo = O.contrastive_loss([oi, od, None], gs["labels"], om.logit_scale.exp())
        ps = [(n, p) for n, p in om.named_parameters() if p.requires_grad]
        go = {n: (torch.zeros_like(p) if g is None else g) for (n, p), g in zip(ps, torch.autograd.grad(lo, [p for _, p in ps], allow_unused=True))}
        # the same oracle with ONE base for all eight rows (the plain step's masks): a different gradient
        with O.dropout(0.1, 0.1, bases[0]):
            od1 = Fn.normalize(om.dna_encoder(gs["dna"]).float(), p=2, dim=-1)
    keys = sorted(got)
    assert sorted(go) == keys
    lo = lo.detach()
    d_emb = max(float((tr.cached_embeddings[0].cpu() - oi.detach()).abs().max()), float((tr.cached_embeddings[1].cpu() - od.detach()).abs().max()))
    d_other = float((tr.cached_embeddings[1].cpu() - od1.detach()).abs().max())
    a, e = whole(got, keys), whole(go, keys)
    print(f"against the oracle chunk by chunk with those bases: embeddings {d_emb:.3e} (DNA rows under one base for the batch: {d_other:.3e}); "
          f"loss off by {abs(float(loss) - float(lo)):.2e}; gradient whole vector rel {rel(a, e):.3e}, cosine {cos(a, e):.6f}")
    assert d_emb < 1e-3 and abs(float(loss) - float(lo)) < 1e-3
    assert d_other > 4 * d_emb                                   # the masks are the chunks' own, not the plain step's
    assert_grads(got, go, rel_tol=0.2, cos_tol=0.98, what="chunked train-mode step vs oracle-bf16 with the chunks' masks")
    assert rel(a, e) < 0.08 and cos(a, e) > 0.997


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------------------
def test_two_chunked_steps_from_the_same_state_are_bit_equal(dev):
    a, b = det_step(dev, 3), det_step(dev, 3, run=1)
    p = det_step(dev, None)
    print(f"two chunked steps (3 + 3 + 2): bucket elements that differ {int((a['g'] != b['g']).sum())}, parameters {int((a['p'] != b['p']).sum())}; "
          f"replay_mismatch {a['mismatch']}, {b['mismatch']}; against the plain step (other dropout masks): rel {rel(a['g'], p['g']):.3e}")
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["g"], b["g"]) and torch.equal(a["p"], b["p"]) and torch.equal(a["rng"], b["rng"])
    assert float(a["g"].abs().max()) > 0 and a["mismatch"] == 0 and b["mismatch"] == 0
    assert not torch.equal(a["g"], p["g"]) and not torch.equal(a["rng"], p["rng"])      # three bases drawn, not one: masks differ by design


# ---- 4. one update per step ----------------------------------------------------------------------------------------------------------------------
def test_clipping_acts_on_the_whole_batch_gradient_and_counts_one_step(dev):
    import optim_reference as OR

    x = det_step(dev, 3, max_grad_norm=1e-3)
    ref, gate, err32 = OR.norm_gate(x["g"].cpu().numpy())
    got, coef = x["grad_norm"], x["coef"]
    err = abs(got - ref) / ref
    print(f"chunked step with max_grad_norm=1e-3: grad_norm {got:.7g}, fp64 norm of the accumulated bucket {ref:.7g}, rel err {err:.3e}, gate {gate:.3e}, coef {coef:.6g}")
    assert err <= gate and coef == float(OR.clip_coef(np.float32(got), 1e-3)) and 0 < coef < 1
    assert x["step_count"] == 1 and x["steps_done"] == 1 and x["mismatch"] == 0
    twin = det_step(dev, 3)                                      # the same step without clipping: the bucket the norm was taken of, bit for bit
    assert torch.equal(x["g"], twin["g"]) and not torch.equal(x["p"], twin["p"])


def test_a_nonfinite_value_in_one_chunk_skips_the_whole_step_and_a_plain_step_follows(dev):
    from clibd_amd.train import Trainer, _towers

    loss_p, grads_p, _, flat_p = plain_step("id", dev)
    model = build("id", dev)
    tr = Trainer(model, lr=1e-3, chunk_size=3, max_grad_norm=1.0, nonfinite="skip")
    before = tr.optimizer.flat_p.clone()
    img, dna, text, labels = batch("id", dev)
    bad = img.clone()
    bad[4, 1, 100, 100] = float("nan")                           # row 4: the second of the chunks 3 + 3 + 2
    loss = tr.step(bad, dna, text, labels)
    torch.cuda.synchronize()
    print(f"NaN in chunk 1: loss {float(loss)}, grad_norm {tr.optimizer.grad_norm.item()}, skipped_steps {int(tr.optimizer.skipped_steps)}, step_count {tr.optimizer.step_count}")
    assert int(tr.optimizer.skipped_steps) == 1 and tr.optimizer.step_count == 1 and torch.equal(tr.optimizer.flat_p, before)
    assert not np.isfinite(tr.optimizer.grad_norm.item()) and not bool(torch.isfinite(tr.optimizer.flat_g).all())
    loss = tr.step(img, dna, text, labels)                       # a clean chunked step moves the parameters again ...
    assert int(tr.optimizer.skipped_steps) == 1 and tr.optimizer.step_count == 2 and not torch.equal(tr.optimizer.flat_p, before)
    assert abs(float(loss) - loss_p) <= 1e-5 and int(tr.replay_mismatch) == 0
    # ... and nothing stale stays behind: the switches of pass 1 and the hooks are back, and a plain Trainer on the same model steps as ever
    for tw in _towers(model):
        assert tw.on_grads_ready is None and (not hasattr(tw, "stack") or tw.stack.train_arithmetic is False)
    with torch.no_grad():
        tr.optimizer.flat_p.copy_(before)                        # the fixture's parameters again (the model's parameters are views of this bucket)
    tr2 = Trainer(model, lr=1e-3)
    assert tr2.chunk_size is None and tr2.replay_mismatch is None
    loss2 = tr2.step(img, dna, text, labels)
    got = named_grads(model)
    print(f"plain step on a second Trainer after the chunked ones: loss {float(loss2):.7f} (fresh plain step {loss_p:.7f})")
    assert abs(float(loss2) - loss_p) <= 1e-5 and tr2.optimizer.step_count == 1
    against_plain(got, grads_p, "plain step after chunked steps")
    assert all(tw.grad_sink is not None and all(v.data_ptr() >= tr2.optimizer.flat_g.data_ptr() for v in tw.grad_sink.values()) for tw in _towers(model))


# ---- 5. SimCLR ---------------------------------------------------------------------------------------------------------------------------------
def test_simclr_chunked_step_matches_plain_step(dev):
    from oracle import clibd_oracle as O
    from clibd_amd.model import create_vit
    from clibd_amd.optim import FusedAdam
    from clibd_amd.simclr import SimCLR, SimCLRViT
    from tests.test_simclr_gpu import _args, _views

    torch.manual_seed(3)
    sd = O.VisionTransformer(img_size=224, patch=16, dim=384, depth=2, heads=6, num_classes=1000).state_dict()
    v1, v2 = _views(torch.Generator().manual_seed(4))
    res = []
    for chunk in (None, 3):
        vit = create_vit("vit_small_patch16_224", num_classes=1000, depth=2)
        vit.load_state_dict(sd, strict=True)
        model = SimCLRViT(vit).to(dev)
        for p in model.parameters():
            p.requires_grad_(True)
        opt = FusedAdam(model.parameters(), lr=1e-2, eps=1.0, weight_decay=1e-4)
        sim = SimCLR(model=model, optimizer=opt, scheduler=None, device=dev, args=_args(), chunk_size=chunk)
        loss = sim.train_step(v1, v2)
        torch.cuda.synchronize()
        res.append((float(loss), int(sim.criterion.last_top1), {n: p.grad.detach().cpu().clone() for n, p in vit.named_parameters()}, sim, opt))
    (lp, tp, gp, sp, op), (lc, tc, gc, sc, oc) = res
    print(f"SimCLR b=4 (8 rows) in chunks of 3 rows: loss {lc:.7f} (plain {lp:.7f}, rel {abs(lc - lp) / abs(lp):.2e}); last_top1 {tc} (plain {tp}); "
          f"replay_mismatch {int(sc.replay_mismatch)}; step_count {oc.step_count}")
    assert abs(lc - lp) <= 1e-5 * abs(lp) and tc == tp and 0 <= tc <= 8
    assert sp.replay_mismatch is None and int(sc.replay_mismatch) == 0 and oc.step_count == op.step_count == 1
    against_plain(gc, gp, "SimCLR chunks of 3 rows")
    assert rel(oc.flat_p, op.flat_p) < 1e-4 and not torch.equal(oc.flat_p, torch.zeros_like(oc.flat_p))


# ---- 6. memory -----------------------------------------------------------------------------------------------------------------------------------
def test_chunked_step_peaks_below_the_plain_step(dev):
    from clibd_amd.train import Trainer

    B = 64
    g = torch.Generator().manual_seed(61)
    img = torch.rand(B, 3, 224, 224, generator=g).to(dev)
    dna = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, 1027, (B, 132), generator=g)], dim=1).to(dev)
    labels = torch.arange(B, device=dev) % 7
    peaks = {}
    for chunk in (None, 8):
        model = build("id", dev, train=True)
        tr = Trainer(model, lr=1e-3, chunk_size=chunk)
        tr.step(img[:8], dna[:8], None, labels[:8])              # weight images and workspaces exist before the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tr.step(img, dna, None, labels)
        torch.cuda.synchronize()
        peaks[chunk] = (torch.cuda.max_memory_allocated(), base)
        del model, tr
    (pp, bp), (pc, bc) = peaks[None], peaks[8]
    print(f"B=64, tiny image+DNA towers: max_memory_allocated plain {pp} B, chunk_size=8 {pc} B, ratio {pc / pp:.3f}; above what was allocated before the "
          f"step: plain {pp - bp} B, chunked {pc - bc} B, ratio {(pc - bc) / (pp - bp):.3f}")
    assert pc < pp


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out, ndev):
    sys.path.insert(0, ROOT)
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
        from clibd_amd.train import Trainer

        res = {}
        for name, kw in (("single", {}), ("bucketed", dict(bucket_bytes=4096))):
            model = build("idt", dev)
            tr = Trainer(model, lr=1e-3, world_size=world, rank=rank, all_gather=True, chunk_size=2, **kw)
            calls, forwards = [], [0]
            real = {k: getattr(dist, k) for k in ("all_gather_into_tensor", "reduce_scatter_tensor", "all_reduce")}
            for k in real:                                     # count this rank's collectives; every record says how many forwards had begun
                setattr(dist, k, (lambda k: lambda t, *a, **kk: (calls.append((k, forwards[0], int(t.numel()))), real[k](t, *a, **kk))[1])(k))
            fwd = model.forward
            model.forward = lambda *a, **kk: (forwards.__setitem__(0, forwards[0] + 1), fwd(*a, **kk))[1]
            try:
                loss = tr.step(*batch("idt", dev, slice(4 * rank, 4 * rank + 4)))
                torch.cuda.synchronize()
            finally:
                for k, f in real.items():
                    setattr(dist, k, f)
                del model.forward
            res[name] = {"loss": float(loss), "grads": named_grads(model, float(world)), "calls": calls, "forwards": forwards[0],
                         "bucketed": tr._bucketed, "bucket": int(tr.optimizer.flat_comm.numel()), "p": tr.optimizer.flat_p.cpu(),
                         "mismatch": int(tr.replay_mismatch), "step_count": tr.optimizer.step_count}
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_two_ranks_chunked_equal_one_process_plain(dev):
    """W = 2 x b = 4 in chunks of 2 against one process at B = 8, plain.  Two processes share the GPU over gloo: no run on more than one GPU exists."""
    import torch.multiprocessing as mp

    loss_p, grads_p, _, _ = plain_step("idt", dev)
    n = torch.cuda.device_count()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_rank_worker, args=(2, 29693, out, n), nprocs=2, join=True)
    res = dict(out)
    assert sorted(res) == [0, 1]
    for name in ("single", "bucketed"):
        for r in (0, 1):
            x = res[r][name]
            kinds = [k for k, _, _ in x["calls"]]
            print(f"{name} rank {r}: loss {x['loss']:.7f} (one process plain {loss_p:.7f}); collectives {x['calls']}; forwards {x['forwards']}; replay_mismatch {x['mismatch']}")
            assert abs(x["loss"] - loss_p) <= 1e-5 and x["mismatch"] == 0 and x["step_count"] == 1 and x["forwards"] == 4
            against_plain(x["grads"], grads_p, f"{name} rank {r} of 2 x 4 in chunks of 2")
            assert kinds.count("all_gather_into_tensor") == 1 and kinds.count("reduce_scatter_tensor") == 1
            reduces = [(at, k) for kind, at, k in x["calls"] if kind == "all_reduce"]
            assert [c[1] for c in x["calls"] if c[0] != "all_reduce"] == [2, 2]            # gather and scatter at the root: after pass 1, before pass 2
            if name == "single":
                assert not x["bucketed"] and reduces == [(4, x["bucket"])]                   # ONE all-reduce: the whole bucket with its aux slots
            else:
                assert x["bucketed"] and len(reduces) > 2 and sum(k for _, k in reduces) == x["bucket"]   # one all-reduce of the bucket, in pieces
                assert all(at == 4 for at, _ in reduces)                                     # none before the last chunk's forward had begun
        assert torch.equal(res[0][name]["p"], res[1][name]["p"])
