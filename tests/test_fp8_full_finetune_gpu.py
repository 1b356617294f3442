"""fp8 forward on the MLP pair (sites fc1_in, fc2_in) with TRAINABLE base weights — full fine-tuning, the reference's 5M recipe
(`disable_lora: true`).  The weight gradients of fc1 and fc2 contract the e4m3 operands the forward GEMMs consumed,
dW = bf16(dY)^T . e4m3(x sa) / sa with fp32 accumulation (ops.gemm_tn_splitk with an e4m3 b, or the dequantising transpose + NT path):
the rows-contracting kernel is checked bit for bit against its bf16 form on the dequantised operand, the towers against an oracle
that states the same rule, and a few training steps against the bf16 forward's gradient."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
MLP = ("fc1_in", "fc2_in")


# ------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("M", [640, 17024])
@pytest.mark.parametrize("Na,Nb", [(3072, 768), (768, 3072), (2048, 512)])
def test_gemm_fp8b_tn_equals_bf16_tn_on_the_dequantised_operand(dev, M, Na, Nb):
    """Products of a bf16 and an e4m3 value are exact in fp32 and a power-of-two factor commutes with every fp32 rounding: the e4m3
    form on (dy, x8, 1/sa) must equal the bf16 form on (dy, bf16(x8 / sa)) BIT FOR BIT — accumulate on / off, column sums on / off,
    the ordered (deterministic) form twice — and both the fp64 product."""
    from clibd_amd import ops

    g = torch.Generator().manual_seed(M + Na + Nb)
    sa = 8.0
    dy = (torch.randn(M, Na, generator=g) * 0.05).bfloat16().to(dev)
    x8 = (torch.randn(M, Nb, generator=g) * sa).clamp(-448, 448).to(FP8).to(dev)
    xb = (x8.float() / sa).bfloat16()
    init = torch.randn(Na, Nb, generator=g).to(dev)
    cs0 = torch.randn(Na, generator=g).to(dev)
    for accumulate, with_cs in ((False, False), (True, False), (False, True), (True, True)):
        o8, o16 = init.clone(), init.clone()
        c8, c16 = (cs0.clone(), cs0.clone()) if with_cs else (None, None)
        assert ops.gemm_tn_splitk(dy, x8, o8, accumulate=accumulate, colsum=c8, b_scale=1.0 / sa)
        assert ops.gemm_tn_splitk(dy, xb, o16, accumulate=accumulate, colsum=c16)
        torch.cuda.synchronize()
        assert torch.equal(o8, o16), (accumulate, with_cs, float((o8 - o16).abs().max()))
        if with_cs:
            assert torch.allclose(c8, c16, rtol=0, atol=1e-3 * float(c16.abs().max()))   # (atomic order)
    ref = dy.double().T @ (x8.double() / sa)
    assert float((o8.double() - init.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-4
    ordered = []
    for _ in range(2):
        o8, c8 = torch.zeros(Na, Nb, device=dev), torch.zeros(Na, device=dev)
        assert ops.gemm_tn_splitk(dy, x8, o8, accumulate=True, colsum=c8, ordered=True, b_scale=1.0 / sa)
        ordered.append((o8.clone(), c8.clone()))
    o16, c16 = torch.zeros(Na, Nb, device=dev), torch.zeros(Na, device=dev)
    assert ops.gemm_tn_splitk(dy, xb, o16, accumulate=True, colsum=c16, ordered=True)
    torch.cuda.synchronize()
    assert torch.equal(ordered[0][0], ordered[1][0]) and torch.equal(ordered[0][1], ordered[1][1])
    assert torch.equal(ordered[0][0], o16) and torch.equal(ordered[0][1], c16)
    assert torch.allclose(c16.double(), dy.double().sum(0), rtol=1e-5, atol=1e-4)


def test_gemm_fp8b_tn_declines_and_validates(dev):
    from clibd_amd import ops

    dy = torch.zeros(200, 768, dtype=torch.bfloat16, device=dev)
    x8 = torch.zeros(200, 512, dtype=torch.uint8, device=dev).view(FP8)
    out = torch.zeros(768, 512, device=dev)
    assert ops.gemm_tn_splitk(dy, x8, out, b_scale=0.5) is False                    # M % 128 != 0: the caller's fallback
    with pytest.raises(ValueError):
        ops.gemm_tn_splitk(dy, x8, out)                                             # an e4m3 b needs its scale
    with pytest.raises(ValueError):
        ops.gemm_tn_splitk(dy, dy[:, :512].contiguous(), out, b_scale=0.5)          # a scale goes with e4m3 only


@pytest.mark.parametrize("R,C,pad", [(2128, 768, 128), (320, 3072, 128), (77, 512, 64)])
def test_transpose_fp8_is_exact(dev, R, C, pad):
    from clibd_amd import ops

    g = torch.Generator().manual_seed(R + C)
    x8 = (torch.randn(R, C, generator=g) * 16).clamp(-448, 448).to(FP8)
    for scale in (0.0625, 0.25):
        got = ops.transpose_fp8(x8.to(dev), scale, pad_to=pad)
        Rp = (R + pad - 1) // pad * pad
        want = torch.zeros(C, Rp, dtype=torch.bfloat16)
        want[:, :R] = (x8.float() * scale).bfloat16().T
        assert got.shape == (C, Rp) and torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------------------- towers vs oracle
def _patch_oracle(monkeypatch, O):
    """The oracle's fp8 linear keeps no weight gradient (its fp8 mode needed frozen weights).  Restated here with the rule of the
    kernels: dW = bf16(dy)^T . e4m3(x sa) / sa, fp32 accumulation; under dgrad8() the 8-bit dgrad's weight gradient takes the same
    dequantised operand (straight-through: the input gradient is unchanged)."""

    class Fp8LinearT(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, weight, sa):
            w8, sn = O.quantize_rows_e4m3(weight.detach().float())
            xq = O.e4m3(x.detach().float() * sa)
            ctx.save_for_backward(weight, xq)
            ctx.sa = sa
            return F.linear(xq, w8) * (1.0 / (sn * sa)).view(-1)

        @staticmethod
        def backward(ctx, dy):
            weight, xq = ctx.saved_tensors
            g = dy.to(torch.bfloat16).to(dy.dtype)
            dw = None
            if weight.requires_grad:
                dw = g.reshape(-1, g.shape[-1]).t() @ (xq / ctx.sa).reshape(-1, xq.shape[-1])
            return g @ weight.detach().to(torch.bfloat16).to(dy.dtype), dw, None

    orig = O.olinear

    def olinear(x, weight, bias=None, round_out=True, fp8_scale=None, dgrad=None):
        if fp8_scale is None:
            return orig(x, weight, bias, round_out, None, dgrad)
        y = Fp8LinearT.apply(x, weight, float(fp8_scale))
        dg = dgrad is not None and O._dg8()
        if dg:
            xq = O.e4m3(x.detach().float() * float(fp8_scale)) / float(fp8_scale)
            y = O._Dgrad8Linear.apply(x + (xq.to(x.dtype) - x).detach(), weight, y.detach(), dgrad[0], id(dgrad[1]))
        if bias is not None:
            y = y + bias
        y = O._r(y) if round_out else y
        return y if dg else O._rg(y)

    monkeypatch.setattr(O, "olinear", olinear)


def _grads(named_params, loss):
    ps = [(n, p) for n, p in named_params if p.requires_grad]
    gs = torch.autograd.grad(loss, [p for _, p in ps], allow_unused=True)
    return {n: (torch.zeros_like(p) if g is None else g).detach().float().cpu() for (n, p), g in zip(ps, gs)}


def _flat(g, names):
    return torch.cat([g[n].flatten().double() for n in names])


def _cos(a, b):
    return float(a @ b / (a.norm() * b.norm()))


def _gate(what, got8, got16, ora):
    live = {n for n, v in ora.items() if float(v.abs().max()) > 0}
    keep = lambda g_: {n: v for n, v in g_.items() if n in live and n in ora}
    g8, g16, go = keep(got8), keep(got16), keep(ora)
    names = sorted(go)
    assert sorted(g8) == names
    assert any("fc1.weight" in n or "intermediate.dense.weight" in n for n in names), names[:8]
    f8, f16, o8 = _flat(g8, names), _flat(g16, names), _flat(go, names)
    big = max(float(go[n].double().norm()) for n in names)
    per = {n: _cos(g8[n].flatten().double(), go[n].flatten().double()) for n in names if float(go[n].double().norm()) > 1e-2 * big}
    worst = min(per, key=per.get)
    print(f"[fp8 MLP forward, full fine-tune, {what}] {len(names)} parameters: cosine vs oracle {_cos(f8, o8):.5f} "
          f"(rel {float((f8 - o8).norm() / o8.norm()):.2e}), worst of {len(per)} large parameters {per[worst]:.4f} ({worst}), "
          f"vs the bf16 forward {_cos(f8, f16):.5f}")
    assert not torch.equal(f8, f16), "the switch did not reach the kernels"
    assert _cos(f8, o8) > 0.999 and per[worst] > 0.985, (what, _cos(f8, o8), per[worst], worst)


def _run_hip(m, stack, x, cot, dev, dgrad8, seed=None):
    """(bf16-forward grads, fp8-MLP-forward grads) of <m(x), cot> with every parameter trainable"""
    out = {}
    for mode in ("bf16", "fp8"):
        stack.disable_fp8()
        if mode == "fp8":
            stack.enable_fp8(sites=MLP)
        stack.set_numerics(dgrad="fp8" if dgrad8 else "bf16")
        if seed is not None:
            torch.manual_seed(seed)
        y = m(x)
        out[mode] = _grads(m.named_parameters(), (y * cot.to(dev)).sum())
    per_layer = stack.fp8
    stack.disable_fp8()
    stack.set_numerics(dgrad="bf16")
    return out, per_layer


@pytest.mark.parametrize("train_mode,dgrad8", [(False, False), (True, False), (False, True)], ids=["eval", "train", "eval+dgrad8"])
def test_fp8_mlp_full_finetune_dna_tower_matches_oracle(dev, monkeypatch, train_mode, dgrad8):
    """BarcodeBERT width (H 768, FF 3072, S 133), 2 layers, batch 16 (M = 2128: the transpose + NT weight-gradient path), every parameter
    trainable; train mode with the HF dropout masks; one case with the 8-bit dgrad on top (its d(fc1 out) bf16 copy is fc1's dY)."""
    from oracle import clibd_oracle as O
    from clibd_amd.data import synthetic_batch
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder

    _patch_oracle(monkeypatch, O)
    torch.manual_seed(41)
    om = O.DNAEncoder(O.BertForMaskedLM(vocab=1027, hidden=768, layers=2, heads=12, ff=3072), 4, 768, lora_layer=[])
    m = CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=1027, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072)), r=4, num_classes=768, lora_layer=[])
    m.load_state_dict(om.state_dict(), strict=True)
    for mod in (om, m):
        for p_ in mod.parameters():
            p_.requires_grad_(True)
    m = m.to(dev).train(train_mode)
    st = m.tower().stack
    assert st.full_mode()
    B = 16
    ids = synthetic_batch(B, torch.device("cpu"), seed=14, rank=0, with_text=False)["dna"]
    cot = torch.randn(B, 768, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(97)
    base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    res, per_layer = _run_hip(m, st, ids.to(dev), cot, dev, dgrad8, seed=97)
    O.set_fp8_scales(om.base_dna_encoder.bert.encoder.layer, per_layer)
    with O.precision("fp8"), (O.dropout(0.1, 0.1, base) if train_mode else contextlib.nullcontext()), O.dgrad8(dgrad8):
        yo = om(ids)
        ora = _grads(om.named_parameters(), (yo * cot).sum())
    _gate(f"DNA {'train' if train_mode else 'eval'}{' + dgrad8' if dgrad8 else ''}", res["fp8"], res["bf16"], ora)


def test_fp8_mlp_full_finetune_text_tower_matches_oracle(dev, monkeypatch):
    """BERT-small (H 512, FF 2048, S 20), batch 32: M = 640, the rows-contracting e4m3 kernel takes every MLP weight gradient."""
    from oracle import clibd_oracle as O
    from clibd_amd.model import BertConfigLite, BertModel, CLIBDLanguageEncoder
    from clibd_amd.model.language_encoder import BERT_SMALL

    _patch_oracle(monkeypatch, O)
    torch.manual_seed(42)
    om = O.LanguageEncoder(O.BertModel(vocab=30522, hidden=512, layers=4, heads=8, ff=2048), r=4, num_classes=768)
    with torch.no_grad():
        for n, p in om.named_parameters():
            if p.dim() >= 2 and "embeddings" not in n:
                p.normal_(0, 0.03)
    m = CLIBDLanguageEncoder(BertModel(BertConfigLite(**BERT_SMALL)), r=4, num_classes=768)
    m.load_state_dict(om.state_dict(), strict=True)
    for mod in (om, m):
        for p_ in mod.parameters():
            p_.requires_grad_(True)
    m = m.to(dev).eval()
    om.eval()
    st = m.tower().stack
    assert st.full_mode()
    g = torch.Generator().manual_seed(9)
    B = 32
    ids = torch.randint(0, 30522, (B, 20), generator=g)
    lens = torch.randint(6, 21, (B,), generator=g)
    x = {"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": (torch.arange(20)[None, :] < lens[:, None]).long()}
    cot = torch.randn(B, 768, generator=g)
    res, per_layer = _run_hip(m, st, {k: v.to(dev) for k, v in x.items()}, cot, dev, False)
    O.set_fp8_scales(om.base_language_encoder.encoder.layer, per_layer)
    with O.precision("fp8"):
        yo = om(x)
        ora = _grads(om.named_parameters(), (yo * cot).sum())
    _gate("text, M = 640", res["fp8"], res["bf16"], ora)


def test_fp8_mlp_full_finetune_image_tower_matches_oracle(dev, monkeypatch):
    """The pre-LN stack: a width-768 ViT of three blocks, batch 16 (two full blocks with the fp8 MLP, the class-row-only last block keeps
    its bf16 remainder), every parameter trainable."""
    from oracle import clibd_oracle as O
    from clibd_amd.model import CLIBDImageEncoder, VisionTransformer

    _patch_oracle(monkeypatch, O)
    torch.manual_seed(43)
    om = O.ImageEncoder(O.VisionTransformer(img_size=224, patch=16, dim=768, depth=3, heads=12, num_classes=0), 4, 768, lora_layer=[])
    with torch.no_grad():
        for n, p in om.named_parameters():
            if "linear_b_" in n:
                p.normal_(0, 0.02)
    m = CLIBDImageEncoder(VisionTransformer(embed_dim=768, depth=3, num_heads=12, num_classes=0), r=4, num_classes=768, lora_layer=[])
    m.load_state_dict(om.state_dict(), strict=True)
    for mod in (om, m):
        for p_ in mod.parameters():
            p_.requires_grad_(True)
    m = m.to(dev).eval()
    st = m.tower().stack
    assert st.full_mode()
    g = torch.Generator().manual_seed(44)
    img, cot = torch.rand(16, 3, 224, 224, generator=g), torch.randn(16, 768, generator=g)
    res, per_layer = _run_hip(m, st, img.to(dev), cot, dev, False)
    O.set_fp8_scales(om.base_image_encoder.blocks, per_layer, last_block_qkv_only=True)
    with O.precision("fp8"):
        yo = om(img)
        ora = _grads(om.named_parameters(), (yo * cot).sum())
    _gate("ViT width 768", res["fp8"], res["bf16"], ora)


# ------------------------------------------------------------------------------------------------------------- training
def _image_dna_model(dev, seed):
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder, CLIBDImageEncoder, SimpleCLIP, VisionTransformer

    torch.manual_seed(seed)
    model = SimpleCLIP(CLIBDImageEncoder(VisionTransformer(embed_dim=768, depth=2, num_heads=12, num_classes=0), r=4, num_classes=768, lora_layer=[]),
                       CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=1027, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072)), r=4, num_classes=768, lora_layer=[]), None)
    for p_ in model.parameters():
        p_.requires_grad_(True)
    return model.to(dev).train()


def _step_grads(model, batch, dev):
    from clibd_amd.model import ClipLoss

    crit = ClipLoss(local_loss=False, gather_with_grad=True, rank=0, world_size=1, criterion=torch.nn.CrossEntropyLoss())
    torch.manual_seed(5)
    hi, hd, _, scale, _ = model(batch["image"], batch["dna"], None)
    loss = crit(hi, hd, None, batch["labels"].to(dev), scale)
    g = _grads(model.named_parameters(), loss)
    names = sorted(g)
    return _flat(g, names)


@pytest.mark.parametrize("dgrad8", [False, True], ids=["bf16-dgrad", "dgrad8-pooled"])
def test_fp8_mlp_full_finetune_trainer(dev, dgrad8):
    """Trainer steps of a small-depth, full-width Image + DNA model, every weight trainable, towers="pooled_ffn", periodic re-calibration:
    the loss is finite and falls, base weights move, and the step's gradient keeps cosine >= 0.98 (the project's training-grade bar)
    against the bf16 forward's on the training batch and on an unseen batch."""
    from clibd_amd.data import synthetic_batch
    from clibd_amd.train import Trainer

    model = _image_dna_model(dev, 45)
    batch = synthetic_batch(16, dev, seed=15, rank=0, with_text=False)
    fresh = synthetic_batch(16, dev, seed=16, rank=0, with_text=False)
    if dgrad8:
        model.enable_fp8_dgrad(towers="pooled")
    cos = {}
    for name, b in (("train", batch), ("fresh", fresh)):
        model.enable_fp8_forward(enabled=False)
        g16 = _step_grads(model, b, dev)
        model.enable_fp8_forward(calibration_inputs=(b["image"], b["dna"], None) if name == "train" else (batch["image"], batch["dna"], None),
                                 towers="pooled_ffn")
        g8 = _step_grads(model, b, dev)
        assert not torch.equal(g8, g16)
        cos[name] = _cos(g8, g16)
    print(f"[fp8 MLP forward, full fine-tune, trainer{' + dgrad8(pooled)' if dgrad8 else ''}] gradient cosine vs the bf16 forward: "
          f"training batch {cos['train']:.5f}, unseen batch {cos['fresh']:.5f}")
    assert cos["train"] >= 0.98 and cos["fresh"] >= 0.98, cos
    st = model.dna_encoder.tower().stack
    assert st.full_mode() and st.fp8 is not None and "qkv_in" not in st.fp8[0]
    assert model.image_encoder.tower().stack.fp8 is None
    tr = Trainer(model, lr=1e-4, world_size=1, rank=0, all_gather=True, fp8_recalibrate_every=2)
    w0 = model.dna_encoder.base_dna_encoder.bert.encoder.layer[0].intermediate.dense.weight.detach().clone()
    losses = [float(tr.step(batch["image"], batch["dna"], None, batch["labels"])) for _ in range(5)]
    print(f"[fp8 MLP forward, full fine-tune, trainer{' + dgrad8(pooled)' if dgrad8 else ''}] losses {losses}")
    assert all(l == l and abs(l) < float("inf") for l in losses) and losses[-1] < losses[0], losses
    assert not torch.equal(w0, model.dna_encoder.base_dna_encoder.bert.encoder.layer[0].intermediate.dense.weight.detach())
    assert st.fp8 is not None and "qkv_in" not in st.fp8[0]        # re-calibration kept the selection


def test_fp8_mlp_full_finetune_deterministic(dev):
    """set_deterministic(True): two full fine-tune steps with the pooled_ffn forward from the same seed are bit-identical.  DNA batch 128
    (M = 17024): the e4m3 rows-contracting kernel in its ordered form."""
    from clibd_amd.data import synthetic_batch
    from clibd_amd.train import Trainer

    runs = []
    for _ in range(2):
        model = _image_dna_model(dev, 46).set_deterministic(True)
        batch = synthetic_batch(128, dev, seed=17, rank=0, with_text=False)
        model.enable_fp8_forward(towers="pooled_ffn")
        tr = Trainer(model, lr=1e-4, world_size=1, rank=0, all_gather=True)
        for _ in range(2):
            tr.step(batch["image"], batch["dna"], None, batch["labels"])
        torch.cuda.synchronize()
        runs.append(torch.cat([p.detach().flatten().cpu() for p in model.parameters()]))
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------------------- boundary
def test_fp8_all_sites_with_trainable_weights_still_raise(dev):
    from clibd_amd.engine import NotSupportedYet

    model = _image_dna_model(dev, 47)
    st = model.dna_encoder.tower().stack
    assert st.full_mode()
    with pytest.raises(NotSupportedYet):
        st.enable_fp8()
    with pytest.raises(NotSupportedYet):
        st.enable_fp8(sites=("qkv_in", "proj_in", "fc1_in", "fc2_in"))
    for towers in ("pooled", "all"):
        with pytest.raises(NotSupportedYet):
            model.enable_fp8_forward(towers=towers)
    st.enable_fp8(sites=MLP)                                                        # the MLP pair is built
    assert st.fp8 is not None and set(st.fp8[0]) == set(MLP)
