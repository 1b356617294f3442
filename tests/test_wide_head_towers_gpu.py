"""BERT towers with 128- and 192-wide heads (the newer BarcodeBERT checkpoints' shapes) on the HIP kernels (GPU): against the bf16-emulating
oracle in eval and train mode (identical dropout masks), under full fine-tuning, against the reference's own fp32 goldens
(tests/golden/wide_head_{128,192}_golden.pt, made by make_wide_head_golden.py), the refusals of what the wide kernels do not build, and one
training step.  (256, 4) is the control at head width 64: the same bodies on the kernels that served every tower before.
Bodies and tolerances are those of tests/test_model_gpu.py for the same fixture type."""
import pytest
import torch

from tests.test_model_gpu import _full_grads, assert_grads, grads_named, load, rel

pytestmark = pytest.mark.gpu

SHAPES = [(256, 4), (256, 2), (384, 2)]      # head widths 64 (control), 128, 192
WIDE = SHAPES[1:]
IDS = [f"h{h}x{n}" for h, n in SHAPES]


def make_pair(hidden, heads, dev, seed, r=4, layers=2):
    """the oracle's DNA encoder with N(0, 0.05) weights and the HIP encoder holding the same state, B = 3, S = 133 token ids"""
    from oracle import clibd_oracle as O
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder

    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    om = O.DNAEncoder(O.BertForMaskedLM(vocab=258, hidden=hidden, layers=layers, heads=heads, ff=2 * hidden), r=r, num_classes=128)
    with torch.no_grad():
        for n, p in om.named_parameters():
            if p.dim() >= 2:
                p.normal_(0, 0.05)
    hm = CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=258, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                                                        intermediate_size=2 * hidden)), r=r, num_classes=128)
    hm.load_state_dict(om.state_dict(), strict=True)
    ids = torch.cat([torch.zeros(3, 1, dtype=torch.long), torch.randint(2, 258, (3, 132), generator=g)], dim=1)
    cot = torch.randn(3, 128, generator=g)
    return hm.to(dev), om, ids, cot


def oracle_grads(om, yo, cot):
    ps = [(n, p) for n, p in om.named_parameters() if p.requires_grad]
    return dict(zip([n for n, _ in ps], torch.autograd.grad((yo * cot).sum(), [p for _, p in ps])))


@pytest.mark.parametrize("hidden,heads", SHAPES, ids=IDS)
def test_eval_mode_matches_oracle(dev, hidden, heads):
    from oracle import clibd_oracle as O

    hm, om, ids, cot = make_pair(hidden, heads, dev, 50 + heads + hidden)
    hm.eval(), om.eval()
    assert hm.tower().stack.dh == hidden // heads
    y = hm(ids.to(dev))
    got = grads_named(hm, (y * cot.to(dev)).sum())
    with O.precision("bf16"):
        yo = om(ids)
        go = oracle_grads(om, yo, cot)
    assert rel(y.cpu(), yo.detach()) < 3e-3, rel(y.cpu(), yo.detach())
    assert_grads(got, go, rel_tol=5e-2, cos_tol=0.998, what=f"{hidden}/{heads} eval")
    with torch.no_grad():                      # the no-grad forward passes no lse: same attention output
        assert rel(hm(ids.to(dev)).cpu(), y.detach().cpu()) < 2e-3


@pytest.mark.parametrize("hidden,heads", SHAPES, ids=IDS)
def test_train_mode_dropout_matches_oracle_masks(dev, hidden, heads):
    from oracle import clibd_oracle as O

    hm, om, ids, cot = make_pair(hidden, heads, dev, 70 + heads + hidden)
    hm.train(), om.eval()
    torch.manual_seed(1234)
    base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(1234)  # the tower draws the same base seed from the CPU generator
    y = hm(ids.to(dev))
    got = grads_named(hm, (y * cot.to(dev)).sum())
    with O.precision("bf16"), O.dropout(0.1, 0.1, base):
        yo = om(ids)
        go = oracle_grads(om, yo, cot)
    assert rel(y.cpu(), yo.detach()) < 4e-3, rel(y.cpu(), yo.detach())
    assert_grads(got, go, rel_tol=3e-2, cos_tol=0.999, what=f"{hidden}/{heads} train-mode vs oracle with identical masks")
    with torch.no_grad():
        ye = hm.eval()(ids.to(dev))
    assert rel(ye.cpu(), y.detach().cpu()) > 1e-4      # and it really is different from eval mode


def test_full_finetune_gradients_at_width_128(dev):
    from oracle import clibd_oracle as O

    hm, om, ids, cot = make_pair(256, 2, dev, 90)
    hm.eval(), om.eval()
    y, yo, got, go = _full_grads(hm, om, lambda mm: mm(ids.to(dev)), lambda oo: oo(ids), cot, dev, O.precision("bf16"))
    assert len(got) > 40 and rel(y.cpu(), yo.detach()) < 4e-3
    assert_grads(got, go, rel_tol=3e-2, cos_tol=0.999, what="dna full fine-tune, head width 128", zero_tol=2e-6, zero_rel=1e-4)


@pytest.mark.parametrize("dh", [128, 192])
def test_towers_against_the_reference_goldens(dev, dh):
    """the HIP tower against the reference's own fp32 evaluation and against the bf16-emulating oracle holding the same weights"""
    from oracle import clibd_oracle as O
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder

    g = load(f"wide_head_{dh}_golden.pt")
    c = g["config"]
    sd = {k: v.float() if v.is_floating_point() else v for k, v in g["state_dict"].items()}
    m = CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=g["vocab"], max_position_embeddings=g["max_pos"], **c)), r=4, num_classes=128)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    om = O.DNAEncoder(O.BertForMaskedLM(vocab=g["vocab"], hidden=c["hidden_size"], layers=c["num_hidden_layers"], heads=c["num_attention_heads"],
                                       ff=c["intermediate_size"], max_pos=g["max_pos"]), r=4, num_classes=128)
    om.load_state_dict(sd, strict=True)
    om.eval()
    y = m(g["ids"].to(dev))
    assert y.shape == (3, 128) and y.dtype == torch.float32 and m.tower().stack.dh == dh
    assert torch.allclose(y.sum(1).cpu(), torch.ones(3), atol=1e-4)
    got = grads_named(m, (y * g["cot"].to(dev)).sum())
    with O.precision("bf16"):
        yo = om(g["ids"])
        go = oracle_grads(om, yo, g["cot"])
    # (2) bf16-emulating oracle: tight
    assert (y.cpu() - yo.detach()).abs().max().item() < 1e-3 * yo.abs().max().item() + 1e-5
    assert rel(y.cpu(), yo.detach()) < 3e-3
    assert_grads(got, go, what=f"wide {dh} vs oracle-bf16")
    # (1) reference fp32 golden: bf16 tolerance
    assert rel(y.cpu(), g["out"]) < 2e-2
    assert_grads(got, g["grads"], rel_tol=5e-2, cos_tol=0.998, what=f"wide {dh} vs reference fp32")


# ---- what the wide kernels do not build ---------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from clibd_amd.engine import NotSupportedYet
    from clibd_amd.model import BertConfigLite, BertModel, CLIBDImageEncoder, CLIBDLanguageEncoder, VisionTransformer
    from clibd_amd.rollout import BarcodeBERTAttentionRollout

    # a key mask on a wide BertTower (the text tower passes one)
    text = CLIBDLanguageEncoder(BertModel(BertConfigLite(vocab_size=1000, hidden_size=256, num_hidden_layers=1, num_attention_heads=2,
                                                         intermediate_size=512)), 4, 128).to(dev).eval()
    ids = torch.randint(0, 1000, (2, 20))
    x = {"input_ids": ids.to(dev), "token_type_ids": torch.zeros_like(ids).to(dev), "attention_mask": torch.ones_like(ids).to(dev)}
    with pytest.raises(NotSupportedYet, match="mask"):
        text(x)
    # a wide ViT
    with pytest.raises(NotSupportedYet, match="head_dim 64 only"):
        CLIBDImageEncoder(VisionTransformer(embed_dim=256, depth=1, num_heads=2, num_classes=10), 4, 128).to(dev).tower()
    # rollout of a wide DNA tower
    hm, _, dna, _ = make_pair(256, 2, dev, 5)
    with pytest.raises(NotSupportedYet, match="head_dim 64"):
        BarcodeBERTAttentionRollout(hm.eval())(dna[:1].to(dev))
    # sequences past the LDS budget at width 192
    h192, _, _, _ = make_pair(384, 2, dev, 6, layers=1)
    with pytest.raises(NotSupportedYet, match="192"):
        h192.eval()(torch.zeros(1, 193, dtype=torch.long, device=dev))


def test_all_site_fp8_is_refused_and_the_mlp_pair_runs(dev):
    from clibd_amd.engine import NotSupportedYet

    hm, _, ids, _ = make_pair(768, 6, dev, 7, layers=1)
    hm.eval()
    stack = hm.tower().stack
    with torch.no_grad():
        y0 = hm(ids.to(dev))
        stack.enable_fp8()
        with pytest.raises(NotSupportedYet, match="e4m3"):
            hm(ids.to(dev))
        stack.enable_fp8(sites=("fc1_in", "fc2_in"))
        y1 = hm(ids.to(dev))
        stack.disable_fp8()
    assert bool(torch.isfinite(y1).all()) and rel(y1.cpu(), y0.cpu()) < 5e-2
    stack.set_numerics(dgrad="fp8")          # the 8-bit dgrad does not touch attention
    y = hm(ids.to(dev))
    got = grads_named(hm, y.square().sum())
    assert all(bool(torch.isfinite(v).all()) for v in got.values()) and any(float(v.abs().max()) > 0 for v in got.values())


def test_one_training_step_with_a_wide_dna_tower(dev):
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder, CLIBDImageEncoder, SimpleCLIP, VisionTransformer
    from clibd_amd.train import Trainer

    torch.manual_seed(0)
    model = SimpleCLIP(CLIBDImageEncoder(VisionTransformer(embed_dim=128, depth=2, num_heads=2, num_classes=10), 4, 128),
                       CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=258, hidden_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                                      intermediate_size=512)), 4, 128), None)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0, 0.05)
    model.to(dev)
    B = 8
    g = torch.Generator().manual_seed(1)
    image = torch.rand(B, 3, 224, 224, generator=g)
    dna = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(2, 258, (B, 132), generator=g)], dim=1)
    trainer = Trainer(model, lr=1e-3, world_size=1, rank=0, all_gather=True)
    before = trainer.optimizer.flat_p.clone()
    loss = trainer.step(image.to(dev), dna.to(dev), None, torch.arange(B).to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    moved = (trainer.optimizer.flat_p - before).abs().max().item()
    assert moved > 0 and bool(torch.isfinite(trainer.optimizer.flat_p).all())
