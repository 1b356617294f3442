"""Deterministic training mode (SimpleCLIP.set_deterministic / Trainer(deterministic=True) / CLIBD_DETERMINISTIC=1).

Full fine-tuning (disable_lora) and LoRA at token counts that are not whole 32-row slabs used to end several reductions in float atomics
(LayerNorm / bias / embedding parameter gradients, the VALU adapter-gradient kernel, generic split-K weight gradients).  With the switch on,
each takes a partials workspace and a fixed-order second kernel: the same parameters, batch and dropout seed give the same bits.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _full_model(dev, seed=11):
    from clibd_amd.model import CLIBDDNAEncoder, CLIBDImageEncoder, SimpleCLIP, create_vit, load_pre_trained_bioscan_bert

    torch.manual_seed(seed)
    model = SimpleCLIP(CLIBDImageEncoder(create_vit("vit_base_patch16_224"), r=4, num_classes=768),
                       CLIBDDNAEncoder(load_pre_trained_bioscan_bert(None), r=4, num_classes=768), None)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "linear_b_" in n or ".w_b." in n:
                p.normal_(0, 0.02)
    for p in model.parameters():
        p.requires_grad_(True)
    return model.to(dev)


def _lora_model(dev, text: bool, seed=11):
    from clibd_amd.model import (CLIBDDNAEncoder, CLIBDImageEncoder, CLIBDLanguageEncoder, SimpleCLIP, create_vit, load_pre_trained_bert,
                                 load_pre_trained_bioscan_bert)

    torch.manual_seed(seed)
    model = SimpleCLIP(CLIBDImageEncoder(create_vit("vit_base_patch16_224"), r=4, num_classes=768),
                       CLIBDDNAEncoder(load_pre_trained_bioscan_bert(None), r=4, num_classes=768),
                       CLIBDLanguageEncoder(load_pre_trained_bert()[1], r=4, num_classes=768) if text else None)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "linear_b_" in n or ".w_b." in n:
                p.normal_(0, 0.02)
    return model.to(dev)


def _trajectory(make, batch, steps=4, **trainer_kw):
    from clibd_amd.train import Trainer

    model = make()
    model.train(True)
    tr = Trainer(model, lr=1e-4, world_size=1, rank=0, all_gather=True, deterministic=True, **trainer_kw)
    assert model.deterministic()
    torch.manual_seed(123)   # the towers draw their dropout base seeds from the CPU generator
    losses = [tr.step(batch["image"], batch["dna"], batch["text"], batch["labels"]).clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), {n: p.detach().clone().cpu() for n, p in model.named_parameters() if p.requires_grad}


def _assert_same(run1, run2):
    (l1, p1), (l2, p2) = run1, run2
    assert torch.isfinite(l1).all(), l1
    assert torch.equal(l1, l2), (l1, l2)
    bad = [n for n in p1 if not torch.equal(p1[n], p2[n])]
    assert not bad, f"{len(bad)} of {len(p1)} trainable tensors differ between two identical runs: {bad[:8]}"


@pytest.mark.parametrize("dgrad", ["bf16", "fp8"])
def test_full_finetune_trajectory_repeats_bit_for_bit(dev, dgrad):
    """Full-size ViT-B/16 + BarcodeBERT, every parameter trainable, B = 32, train mode (dropout), four AdamW steps, twice from fresh models."""
    from clibd_amd.data import synthetic_batch

    batch = synthetic_batch(32, dev, seed=3, rank=0, with_text=False)
    make = lambda: _full_model(dev).enable_fp8_dgrad("all", enabled=(dgrad == "fp8"))
    _assert_same(_trajectory(make, batch), _trajectory(make, batch))


def test_odd_batch_lora_trajectory_repeats_bit_for_bit(dev):
    """Tri-modal LoRA at B = 20: 3 940 ViT rows, 2 660 DNA rows, 400 text rows (padding masks) — none a whole number of 32-row slabs."""
    from clibd_amd.data import synthetic_batch

    batch = synthetic_batch(20, dev, seed=5, rank=0, with_text=True)
    make = lambda: _lora_model(dev, text=True)
    _assert_same(_trajectory(make, batch), _trajectory(make, batch))


def _step_grads(model, batch, deterministic: bool):
    from clibd_amd.model import ClipLoss

    model.set_deterministic(deterministic)
    ps = {n: p for n, p in model.named_parameters() if p.requires_grad}
    crit = ClipLoss(local_loss=False, gather_with_grad=True, rank=0, world_size=1, criterion=torch.nn.CrossEntropyLoss())
    hi, hd, ht, scale, _ = model(batch["image"], batch["dna"], batch["text"])
    loss = crit(hi, hd, ht, batch["labels"], scale)
    gs = torch.autograd.grad(loss, list(ps.values()), allow_unused=True)
    model.join_streams()
    torch.cuda.synchronize()
    return {n: (torch.zeros_like(p) if g is None else g.detach().clone()) for (n, p), g in zip(ps.items(), gs)}


@pytest.mark.parametrize("setup", ["full_b32", "lora_trimodal_b20"])
def test_switch_changes_only_the_summation_order(dev, setup):
    from clibd_amd.data import synthetic_batch

    if setup == "full_b32":
        model, batch = _full_model(dev).eval(), synthetic_batch(32, dev, seed=6, rank=0, with_text=False)
    else:
        model, batch = _lora_model(dev, text=True).eval(), synthetic_batch(20, dev, seed=6, rank=0, with_text=True)
    g_off = _step_grads(model, batch, False)
    g_on = _step_grads(model, batch, True)
    bad = []
    for n in g_off:
        a, b = g_off[n].double(), g_on[n].double()
        fa, fb = torch.isfinite(a), torch.isfinite(b)
        if not torch.equal(fa, fb):
            bad.append((n, "non-finite pattern"))
            continue
        d = (a[fa] - b[fb]).norm() / max(a[fa].norm().item(), 1e-30)
        if d > 1e-5:
            bad.append((n, float(d)))
    assert not bad, bad[:8]


def test_whole_slab_lora_is_unchanged_by_the_switch(dev):
    """B = 32 under LoRA (6 304 / 4 256 token rows: whole slabs): the switch launches the same kernels, so the bits are identical."""
    from clibd_amd.data import synthetic_batch

    model = _lora_model(dev, text=False).eval()
    batch = synthetic_batch(32, dev, seed=7, rank=0, with_text=False)
    g_off = _step_grads(model, batch, False)
    g_on = _step_grads(model, batch, True)
    bad = [n for n in g_off if not torch.equal(g_off[n], g_on[n])]
    assert not bad, bad[:8]


class _Recorder:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("clibd_") or not callable(fn):
            return fn

        def wrapped(*args):
            self.calls.append((name, args))
            return fn(*args)

        return wrapped


def test_no_atomic_form_is_reached(dev, monkeypatch):
    """One deterministic full fine-tune step (8-bit dgrad on both towers, so that both LayerNorm parameter-gradient kernels run) and one
    tri-modal LoRA step at B = 20: every reduction call carries its partials workspace (a NULL workspace selects the float atomics)."""
    from clibd_amd import _lib
    from clibd_amd.data import synthetic_batch

    real = _lib.load()
    rec = _Recorder(real)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    reductions = {"clibd_colsum_bf16", "clibd_batch_sum_f32", "clibd_bert_embed_bwd", "clibd_layernorm_param_grads", "clibd_transpose_colsum_bf16"}
    for model, batch in ((_full_model(dev).enable_fp8_dgrad("all").eval(), synthetic_batch(32, dev, seed=8, rank=0, with_text=False)),
                         (_lora_model(dev, text=True).eval(), synthetic_batch(20, dev, seed=8, rank=0, with_text=True))):
        rec.calls.clear()
        _step_grads(model, batch, True)
        names = [n for n, _ in rec.calls]
        assert "clibd_attention_bwd" in names, sorted(set(names))
        for n, a in rec.calls:
            if n in reductions:   # (..., workspace, workspace_bytes, stream)
                assert a[-3] is not None and a[-2] > 0, f"{n} without a partials workspace"
            if n == "clibd_layernorm_bwd" and a[17] is not None:   # dgamma
                assert a[19] is not None and a[20] > 0, "LayerNorm parameter gradients without a workspace"
            if n in ("clibd_gemm_bf16_tn_splitk", "clibd_gemm_fp8b_tn_splitk") and a[-6] is not None:   # colsum_a
                assert a[-3] is not None and a[-2] > 0, "TN split-K with a bias column sum and no colsum workspace"
            if n == "clibd_gemm_bf16_nt":
                assert a[7]._obj.split_k <= 1, "generic split-K (atomic) weight gradient"
            if n in ("clibd_lora_backward", "clibd_lora_wgrad"):
                assert a[-3] is not None and a[-2] > 0, "adapter gradients without a partials workspace"


# ---- op level: each ordered form, three runs on the same inputs: identical bits, and the float64 sum within 1e-5 relative -------------
def _three(fn):
    outs = [fn() for _ in range(3)]
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    return outs[0]


def _close(got, ref, tol=1e-5):
    got, ref = got.double().cpu(), ref.double().cpu()
    rel = (got - ref).norm() / max(ref.norm().item(), 1e-30)
    assert rel <= tol, float(rel)


def test_ordered_layernorm_bwd_param_grads(dev):
    from clibd_amd import ops

    M, H = 50432, 768
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(M, H, generator=g).to(dev)
    gamma, beta = (1 + 0.1 * torch.randn(H, generator=g)).to(dev), torch.zeros(H, device=dev)
    dy = torch.randn(M, H, generator=g).to(dev).to(torch.bfloat16)
    st = torch.empty((M, 2), device=dev)
    ops.layernorm_fwd(x, gamma, beta, 1e-6, y_f32=torch.empty_like(x), stats=st)

    def run():
        dg, db = torch.zeros(H, device=dev), torch.zeros(H, device=dev)
        ops.layernorm_bwd(dy, x, st, gamma, dx_bf16=torch.empty((M, H), dtype=torch.bfloat16, device=dev), dgamma=dg, dbeta=db, ordered=True)
        return torch.cat([dg, db])

    out = _three(run)
    xhat = (x.double() - st[:, :1].double()) * st[:, 1:].double()
    _close(out, torch.cat([(dy.double() * xhat).sum(0), dy.double().sum(0)]))


@pytest.mark.parametrize("kind", ["uniform", "one_id", "text_padding"])
def test_ordered_bert_embed_bwd(dev, kind):
    from clibd_amd import ops

    V, H = 30522, 768
    g = torch.Generator(device="cpu").manual_seed(2)
    if kind == "uniform":
        ids = torch.randint(0, V, (2048 * 20,), generator=g)
    elif kind == "one_id":
        ids = torch.full((4096,), 7, dtype=torch.int64)
    else:
        lens = torch.randint(6, 21, (2048,), generator=g)
        ids = torch.randint(1000, V, (2048, 20), generator=g)
        ids[torch.arange(20)[None] >= lens[:, None]] = 0
        ids[:, 0] = 101
        ids = ids.reshape(-1)
    M = ids.numel()
    tt = (torch.rand(M, generator=g) < 0.1).long()
    de = torch.randn(M, H, generator=g)
    ids_d, tt_d, de_d = ids.to(dev), tt.to(dev), de.to(dev)

    def run():
        dw, dt = torch.zeros((V, H), device=dev), torch.zeros((2, H), device=dev)
        ops.bert_embed_bwd(ids_d, tt_d, de_d, dw, dt, ordered=True)
        return torch.cat([dw, dt])

    out = _three(run).cpu()
    ref_w = torch.zeros((V, H), dtype=torch.float64).index_add_(0, ids, de.double())
    ref_t = torch.zeros((2, H), dtype=torch.float64).index_add_(0, tt, de.double())
    _close(out[:V], ref_w)
    _close(out[V:], ref_t)


def test_ordered_batch_sum_colsum_and_tn(dev):
    from clibd_amd import ops

    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(2048, 197 * 8, generator=g).to(dev)
    _close(_three(lambda: (lambda o: (ops.batch_sum(x, o, ordered=True), o)[1])(torch.zeros(197 * 8, device=dev))), x.double().sum(0))
    y = torch.randn(20000, 320, generator=g).to(dev).to(torch.bfloat16)
    _close(_three(lambda: (lambda o: (ops.colsum_bf16(y, o, ordered=True), o)[1])(torch.zeros(320, device=dev))), y.double().sum(0))
    M, Na, Nb = 6272, 768, 768
    a = (0.1 * torch.randn(M, Na, generator=g)).to(dev).to(torch.bfloat16)
    b = (0.1 * torch.randn(M, Nb, generator=g)).to(dev).to(torch.bfloat16)

    def tn():
        out, cs = torch.zeros((Na, Nb), device=dev), torch.zeros(Na, device=dev)
        assert ops.gemm_tn_splitk(a, b, out, accumulate=True, colsum=cs, ordered=True)
        return torch.cat([out.view(-1), cs])

    got = _three(tn)
    _close(got[Na * Nb:], a.double().sum(0))
    _close(got[:Na * Nb], (a.double().t() @ b.double()).view(-1), tol=1e-4)


def test_ordered_lora_at_ragged_m(dev):
    from clibd_amd import ops

    M, H = 6299, 768
    g = torch.Generator(device="cpu").manual_seed(4)
    dqkv = (0.1 * torch.randn(M, 3 * H, generator=g)).to(dev).to(torch.bfloat16)
    x = torch.randn(M, H, generator=g).to(dev).to(torch.bfloat16)
    t = torch.randn(M, 8, generator=g).to(dev).to(torch.bfloat16)
    w_dt = (0.1 * torch.randn(16, 3 * H, generator=g)).to(dev).to(torch.bfloat16)

    def run():
        dt = torch.empty((M, 16), dtype=torch.bfloat16, device=dev)
        gs = [torch.zeros((4, H), device=dev), torch.zeros((4, H), device=dev), torch.zeros((H, 4), device=dev), torch.zeros((H, 4), device=dev)]
        ops.lora_backward(dqkv, x, t, w_dt, dt, *gs, ordered=True)
        return torch.cat([dt.float().view(-1)] + [q.view(-1) for q in gs])

    out = _three(run)
    # the same sums through the unpadded VALU kernel (float atomics): the reference arithmetic, another summation order
    dt = torch.empty((M, 16), dtype=torch.bfloat16, device=dev)
    gs = [torch.zeros((4, H), device=dev), torch.zeros((4, H), device=dev), torch.zeros((H, 4), device=dev), torch.zeros((H, 4), device=dev)]
    ops.lora_backward(dqkv, x, t, w_dt, dt, *gs, workspace=False)
    ref = torch.cat([dt.float().view(-1)] + [q.view(-1) for q in gs])
    assert torch.equal(out[:M * 16], ref[:M * 16])
    _close(out[M * 16:], ref[M * 16:])
    _close(out[M * 16:], torch.cat([q.view(-1) for q in _lora_grads_f64(dqkv, x, t, dt, H)]), tol=1e-4)


def _lora_grads_f64(dqkv, x, t, dt, H):
    """float64 adapter gradients of the rank-(4+4) slot: dA_q = dt_q^T x, dA_v = dt_v^T x, dB_q = dq^T t_q, dB_v = dv^T t_v"""
    dq, dv, xd, td, dtd = dqkv[:, :H].double(), dqkv[:, 2 * H:].double(), x.double(), t.double(), dt.double()
    return [dtd[:, 0:4].t() @ xd, dtd[:, 4:8].t() @ xd, dq.t() @ td[:, 0:4], dv.t() @ td[:, 4:8]]


# ---- the workspace forms at the smallest shapes that cross each cap of the partial count (where a wrong grid would overrun the workspace) ----
def _ln_param_inputs(M, H):
    g = torch.Generator(device="cpu").manual_seed(M + H)
    x = torch.randn(M, H, generator=g) * 2 + 0.5
    dy = torch.randn(M, H, generator=g)
    mean = x.double().mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(1, unbiased=False, keepdim=True) + 1e-12)
    return x, dy, torch.cat([mean, rstd], dim=1).float()


@pytest.mark.parametrize("M,H,f32dy,drop", [(65536 + 70, 64, False, False), (65536 + 70, 64, True, False), (70, 128, False, False), (70, 128, True, False),
                                            (65536 + 70, 64, False, True)])
def test_ordered_layernorm_param_grads(dev, M, H, f32dy, drop):
    """(65536 + 70, 64): 1026 row chunks on the 1024 blocks of the workspace form, so two blocks make a second grid-stride sweep, the last chunk
    ragged (6 rows); (70, 128): two blocks, the last ragged."""
    from clibd_amd import ops
    from oracle import clibd_oracle as O

    x, dy, stats = _ln_param_inputs(M, H)
    dyd = dy.to(dev) if f32dy else dy.to(dev, torch.bfloat16)
    xd, std = x.to(dev), stats.to(dev)
    d = ops.Drop(0.1, 99) if drop else None

    def run():
        dg, db = torch.zeros(H, device=dev), torch.zeros(H, device=dev)
        ops.layernorm_param_grads(dyd, xd, std, dg, db, drop=d, ordered=True)
        return torch.cat([dg, db])

    out = _three(run)
    dyr = dyd.double().cpu()
    if drop:
        idx = torch.arange(M, dtype=torch.int64)[:, None] * H + torch.arange(H, dtype=torch.int64)[None, :]
        dyr = dyr * O.drop_factor(99, idx, 0.1).double()
    xhat = (x.double() - stats[:, :1].double()) * stats[:, 1:].double()
    _close(out[:H], (dyr * xhat).sum(0))
    _close(out[H:], dyr.sum(0))


def _colsum_input():
    return torch.randn(65536 + 257, 64, generator=torch.Generator(device="cpu").manual_seed(5)).to(torch.bfloat16)


def test_ordered_colsum_beyond_the_row_cap(dev):
    """65 793 rows: 258 chunks of 256 rows on the 256 partial rows of the workspace form (a second sweep, the last chunk one row)."""
    from clibd_amd import ops

    y = _colsum_input().to(dev)
    _close(_three(lambda: (lambda o: (ops.colsum_bf16(y, o, ordered=True), o)[1])(torch.zeros(64, device=dev))), y.double().sum(0))


def _batch_sum_input(B):
    return torch.randn(B, 300, generator=torch.Generator(device="cpu").manual_seed(B))


@pytest.mark.parametrize("B", [63, 64, 70])
def test_ordered_batch_sum_chunking(dev, B):
    """B = 63: one chunk; 64: eight chunks of 8 rows; 70: eight chunks of 9 rows, the last holding 7."""
    from clibd_amd import ops

    x = _batch_sum_input(B).to(dev)
    _close(_three(lambda: (lambda o: (ops.batch_sum(x, o, ordered=True), o)[1])(torch.zeros(300, device=dev))), x.double().sum(0))


def _tn_inputs(M, Na, Nb, fp8):
    g = torch.Generator(device="cpu").manual_seed(M + Na + (1 if fp8 else 0))
    a = (0.1 * torch.randn(M, Na, generator=g)).to(torch.bfloat16)
    b = torch.randn(M, Nb, generator=g)
    return a, (b.to(torch.float8_e4m3fn) if fp8 else (0.1 * b).to(torch.bfloat16))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("M", [256, 1024])
def test_ordered_tn_splitk_colsum_slices(dev, M, fp8):
    """One output tile (Na = Nb = 256).  M = 256: one slice; M = 1024: several slices of that tile, the column sums one partial per slice."""
    from clibd_amd import ops

    Na = Nb = 256
    a, b = _tn_inputs(M, Na, Nb, fp8)
    ad, bd = a.to(dev), b.to(dev)
    scale = dict(b_scale=0.5) if fp8 else {}

    def tn():
        out, cs = torch.zeros((Na, Nb), device=dev), torch.zeros(Na, device=dev)
        assert ops.gemm_tn_splitk(ad, bd, out, accumulate=True, colsum=cs, ordered=True, **scale)
        return torch.cat([out.view(-1), cs])

    got = _three(tn)
    bref = b.float().double() * (0.5 if fp8 else 1.0)
    _close(got[Na * Nb:], a.double().sum(0))
    _close(got[:Na * Nb], (a.double().t() @ bref).view(-1), tol=1e-4)
