"""GPU checks of the pre-extracted-feature towers (clibd_amd.towers.MLPTower, include/clibd_hip_mlp.h): each role of the one-launch
fp32-grade linear kernel and the whole tower against fp64 torch on the CPU, the ReLU mask rule on exact zeros, the accumulate flag and
run-to-run bits, the composed `linear_f32_*` + ReLU tower as a second yardstick, a 20-step `Trainer` trajectory against the reference's
modules under torch.optim.AdamW (tests/golden/mlp_towers_golden.pt), the eval loop, and checkpoints.

Gates: rel_err (the norm ratio of tests/test_method_linear_gpu.py) < 1e-4 for outputs, dh, every dW and db — the project's fp32-grade gate: a CPU
emulation of the three-term split product through all three layers, forward and backward, sits at 5.8e-6 .. 7.9e-6 and one plain bf16
product at 3e-3 .. 6e-2.  Trajectory: every loss within 2e-4 |ref| + 1e-3 of the reference's, final weights at rel_err < 1e-3.

Mask bits: a pre-activation within the arithmetic's rounding (~1e-6) of 0 may take the other side of the ReLU than fp64 does, and one
flipped bit moves a whole element of dh: 1 / sqrt(elements) of its norm (6.2e-3 at 77 x 64, measured on the first fixture, which held a
pre-activation of 2.4e-6), in any correct implementation.  So the data of the tower cases and of the fixture keeps every pre-activation
at least 1e-4 from 0 (make_mlp_towers_golden.keep_preactivations_off_zero moves hidden biases by <= 0.05 and asserts the room).

Measured on an MI355X (the figures these tests print): per role, all six shapes: forward, dgrad and dW rel_err <= 5.0e-6, db <= 1.3e-7;
whole tower: out 3.4e-6 .. 5.4e-6, dW 6.1e-6 .. 7.8e-6, db 9e-8 .. 7.4e-6; the trajectory's losses 9.66580 -> 1.96420 against the reference's
9.66581 -> 1.96420 (worst |diff| 2.6e-3 of the gate), final weights 1.1e-6 .. 2.5e-6; eval embeddings 6.1e-6; new against composed <= 2.7e-6.

Shapes (B, in, hid, out): one tile with a K tail of 4 (1, 4, 16, 16); tiles that end inside a block (77, 64, 64, 64); the 500-wide INSECT
DNA features, K tail 20 and N tails 48, 80 (130, 500, 48, 80); more than one block each way (257, 192, 64, 128); many K steps and
N = 192, 320 = 3 and 5 tiles (65, 1024, 192, 320); one workload-shaped case (512, 768, 512, 512)."""
import functools
import importlib.util
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(1, 4, 16, 16), (77, 64, 64, 64), (130, 500, 48, 80), (257, 192, 64, 128), (65, 1024, 192, 320), (512, 768, 512, 512)]
COMPOSED_SHAPES = [s for s in SHAPES if s[1] % 64 == 0 and s[2] % 64 == 0]      # clibd_linear_f32_* takes contractions that are multiples of 64
GATE = 1e-4
NAMES = [f"encoder.{j}.{n}" for j in (0, 2, 4) for n in ("weight", "bias")]


def rel_err(a, b):      # as in tests/test_method_linear_gpu.py
    return ((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30)).item()


def loss_close(got, ref):
    return abs(got - ref) < 2e-4 * abs(ref) + 1e-3


@functools.lru_cache(maxsize=None)
def _gen():
    spec = importlib.util.spec_from_file_location("make_mlp_towers_golden", ROOT / "tests" / "golden" / "make_mlp_towers_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _golden():
    return torch.load(ROOT / "tests" / "golden" / "mlp_towers_golden.pt", weights_only=False)


@functools.lru_cache(maxsize=None)
def case(shape):
    """seeded weights (torch's default Linear initialisation, biases widened so that they matter), inputs and the fp64 results, computed
    once per shape and shared by every test; nothing writes to it"""
    B, i, h, o = shape
    g = torch.Generator().manual_seed(B * 7919 + i)
    torch.manual_seed(B * 31 + o)
    seq = torch.nn.Sequential(torch.nn.Linear(i, h), torch.nn.ReLU(), torch.nn.Linear(h, h), torch.nn.ReLU(), torch.nn.Linear(h, o))
    sd = {f"encoder.{k}": v.detach().clone() for k, v in seq.state_dict().items()}
    for j in (0, 2, 4):
        sd[f"encoder.{j}.bias"] = 0.2 * torch.randn(sd[f"encoder.{j}.bias"].shape, generator=g)
    x, dout = torch.randn(B, i, generator=g), torch.randn(B, o, generator=g)
    sd = _gen().keep_preactivations_off_zero(sd, x)      # every pre-activation at least 1e-4 from 0: the fp64 masks are the kernels' masks
    return dict(sd=sd, x=x, dout=dout, **_gen().tower_fp64(sd, x, dout))


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


def encoder(sd, dev):
    from clibd_amd.model import MLPEncoder

    h, i = sd["encoder.0.weight"].shape
    enc = MLPEncoder(i, h, sd["encoder.4.weight"].shape[0])
    enc.load_state_dict(sd)
    return enc.to(dev)


def tower_grads(enc, x, dout):
    out = enc(x)
    out.backward(dout)
    grads = {n: p.grad.clone() for n, p in enc.named_parameters()}
    for p in enc.parameters():
        p.grad = None
    return out.detach(), grads


# ---- the three roles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_each_role_against_fp64(ops, dev, shape):
    """layer 1 (K = in, N = hid) and layer 3 (K = hid, N = out) of the case: forward with and without ReLU and bias, dgrad with and
    without the mask, wgrad with db"""
    c = case(shape)
    B = shape[0]
    g = torch.Generator().manual_seed(5)
    for wn, bn in (("encoder.0.weight", "encoder.0.bias"), ("encoder.4.weight", "encoder.4.bias")):
        w, b = c["sd"][wn], c["sd"][bn]
        N, K = w.shape
        x, dy = torch.randn(B, K, generator=g), torch.randn(B, N, generator=g)
        h = torch.relu(torch.randn(B, K, generator=g))                       # about half exact zeros
        pre = x.double() @ w.double().T
        ref = {"fwd": pre + b.double(), "fwd_relu": torch.relu(pre + b.double()), "fwd_nobias_relu": torch.relu(pre),
               "dgrad": dy.double() @ w.double(), "dgrad_mask": (dy.double() @ w.double()) * (h > 0), "dw": dy.double().T @ x.double(),
               "db": dy.double().sum(0)}
        xd, wd, bd, dyd, hd = (t.to(dev) for t in (x, w, b, dy, h))
        dw, db = ops.mlp_linear_wgrad(dyd, xd)
        dw_only, none = ops.mlp_linear_wgrad(dyd, xd, need_db=False)
        got = {"fwd": ops.mlp_linear_fwd(xd, wd, bd), "fwd_relu": ops.mlp_linear_fwd(xd, wd, bd, relu=True),
               "fwd_nobias_relu": ops.mlp_linear_fwd(xd, wd, None, relu=True), "dgrad": ops.mlp_linear_dgrad(dyd, wd),
               "dgrad_mask": ops.mlp_linear_dgrad(dyd, wd, hd), "dw": dw, "db": db}
        assert none is None and torch.equal(dw_only, dw)
        for name, r in ref.items():
            e = rel_err(got[name], r)
            print(f"{shape} {wn} {name}: rel_err {e:.3e}")
            assert got[name].shape == r.shape and e < GATE, (shape, wn, name, e)
        assert (got["dgrad_mask"][hd == 0] == 0).all() and (got["fwd_relu"] >= 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_whole_tower_against_fp64(dev, shape):
    c = case(shape)
    enc = encoder(c["sd"], dev)
    out, grads = tower_grads(enc, c["x"].to(dev), c["dout"].to(dev))
    e = rel_err(out, c["out"])
    print(f"{shape} out: rel_err {e:.3e}")
    assert e < GATE, (shape, e)
    for n in NAMES:
        e = rel_err(grads[n], c["grads"][n])
        print(f"{shape} d {n}: rel_err {e:.3e}")
        assert grads[n].shape == c["grads"][n].shape and e < GATE, (shape, n, e)
    # the no-grad (eval) forward saves nothing and returns the same bits
    with torch.no_grad():
        assert torch.equal(enc(c["x"].to(dev)), out)
    out_t, state = enc.tower()._forward((c["x"].to(dev),), False)
    assert state is None and torch.equal(out_t, out)


def test_golden_tower_outputs_gradients_and_dh(ops, dev):
    """the fixture's tower (the reference's MLPEncoder, its weights, fp64 results): out, every parameter gradient, and the two dgrad
    launches' outputs dh2, dh1 through the ops"""
    t = _golden()["tower"]
    enc = encoder(t["state_dict"], dev)
    x, dout = t["x"].to(dev), t["dout"].to(dev)
    out, grads = tower_grads(enc, x, dout)
    w2, w3 = enc.encoder[2].weight.detach(), enc.encoder[4].weight.detach()
    _, (xs, h1, h2) = enc.tower()._forward((x,), True)
    dh2 = ops.mlp_linear_dgrad(dout, w3, h2)
    dh1 = ops.mlp_linear_dgrad(dh2, w2, h1)
    got = dict(out=out, dh2=dh2, dh1=dh1, **{"d " + n: grads[n] for n in NAMES})
    ref = dict(out=t["out"], dh2=t["dh2"], dh1=t["dh1"], **{"d " + n: t["grads"][n] for n in NAMES})
    for n in got:
        e = rel_err(got[n], ref[n])
        print(f"golden tower {n}: rel_err {e:.3e}")
        assert e < GATE, (n, e)


def test_relu_mask_rule_on_exact_zeros(ops, dev):
    """A layer whose pre-activation is exactly 0 in columns 0..7 (zero weights, zero bias), negative in 8..15 (bias -1) and positive in
    16..47: h > 0 is torch's ReLU backward, so the gradient into columns 0..15 is an exact zero and the others are the plain product."""
    B, K0, H, N = 70, 32, 48, 32
    g = torch.Generator().manual_seed(11)
    w1, b1 = torch.randn(H, K0, generator=g), torch.zeros(H)
    w1[:16] = 0
    b1[8:16] = -1.0
    b1[16:] = 40.0                                                         # |x w1^T| stays far below 40: positive everywhere
    x, dy, w2 = torch.randn(B, K0, generator=g), torch.randn(B, N, generator=g), torch.randn(N, H, generator=g)
    h = ops.mlp_linear_fwd(x.to(dev), w1.to(dev), b1.to(dev), relu=True)
    assert (h[:, :16] == 0).all() and (h[:, 16:] > 0).all()
    dx = ops.mlp_linear_dgrad(dy.to(dev), w2.to(dev), h)
    assert (dx[:, :16] == 0).all() and (dx[:, 16:] != 0).all()
    assert rel_err(dx[:, 16:], (dy.double() @ w2.double())[:, 16:]) < GATE
    # the same through the tower: d W1 and d b1 of the dead units are exact zeros
    enc = encoder({"encoder.0.weight": w1, "encoder.0.bias": b1, "encoder.2.weight": w2[:, :H].repeat(2, 1)[:H], "encoder.2.bias": torch.zeros(H),
                   "encoder.4.weight": torch.randn(16, H, generator=g), "encoder.4.bias": torch.zeros(16)}, dev)
    _, grads = tower_grads(enc, x.to(dev), torch.randn(B, 16, generator=g).to(dev))
    assert (grads["encoder.0.weight"][:16] == 0).all() and (grads["encoder.0.bias"][:16] == 0).all()
    assert (grads["encoder.0.weight"][16:].abs().sum(1) > 0).all()


@pytest.mark.parametrize("shape", [(130, 500, 48, 80), (257, 192, 64, 128)], ids=str)
def test_accumulate_flag_and_repeatable_bits(ops, dev, shape):
    """accumulate: a pre-filled sink ends at prefill + fresh; through the tower's grad_sink (the trainer's flat bucket) the same.  Two
    identical backward calls give the same bits in every dW and db."""
    c = case(shape)
    enc = encoder(c["sd"], dev)
    x, dout = c["x"].to(dev), c["dout"].to(dev)
    _, fresh = tower_grads(enc, x, dout)
    _, again = tower_grads(enc, x, dout)
    for n in NAMES:
        assert torch.equal(fresh[n], again[n]), n
    g = torch.Generator().manual_seed(3)
    params = dict(enc.named_parameters())
    prefill = {n: torch.randn(params[n].shape, generator=g).to(dev) for n in NAMES}
    sink = {id(params[n]): prefill[n].clone() for n in NAMES}
    tw = enc.tower()
    tw.grad_sink = sink
    try:
        enc(x).backward(dout)
    finally:
        tw.grad_sink = None
    for n in NAMES:
        assert params[n].grad is None
        got = sink[id(params[n])]
        e = rel_err(got - prefill[n], fresh[n])
        print(f"{shape} sink {n}: rel_err of (got - prefill) to fresh {e:.3e}")
        assert rel_err(got, prefill[n] + fresh[n]) < GATE and e < GATE, (n, e)
    # the op itself: one fp32 add of the fresh value to what the buffer held
    dy, a = dout, tw._forward((x,), True)[1][2]
    dw0, db0 = ops.mlp_linear_wgrad(dy, a)
    dw1, db1 = prefill["encoder.4.weight"].clone(), prefill["encoder.4.bias"].clone()
    ops.mlp_linear_wgrad(dy, a, dw1, db1, accumulate=True)
    assert torch.equal(dw1, prefill["encoder.4.weight"] + dw0) and torch.equal(db1, prefill["encoder.4.bias"] + db0)


@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=str)
def test_against_the_composed_linear_f32_tower(ops, dev, shape):
    """the same tower composed from the linear-probe head's clibd_linear_f32_fwd / _bwd (operand images, transposes, K-tripled GEMMs)
    and torch's ReLU: the two fp32-grade paths agree within the gate each way"""
    c = case(shape)
    enc = encoder(c["sd"], dev)
    x, dout = c["x"].to(dev), c["dout"].to(dev)
    out, grads = tower_grads(enc, x, dout)
    w = [c["sd"][f"encoder.{j}.weight"].to(dev) for j in (0, 2, 4)]
    b = [c["sd"][f"encoder.{j}.bias"].to(dev) for j in (0, 2, 4)]
    h1 = torch.relu(ops.linear_f32_fwd(x, w[0], b[0]))
    h2 = torch.relu(ops.linear_f32_fwd(h1, w[1], b[1]))
    comp = {"out": ops.linear_f32_fwd(h2, w[2], b[2])}
    dh2, comp["d encoder.4.weight"], comp["d encoder.4.bias"] = ops.linear_f32_bwd(dout, h2, w[2])
    dh2 = dh2 * (h2 > 0)
    dh1, comp["d encoder.2.weight"], comp["d encoder.2.bias"] = ops.linear_f32_bwd(dh2, h1, w[1])
    dh1 = dh1 * (h1 > 0)
    _, comp["d encoder.0.weight"], comp["d encoder.0.bias"] = ops.linear_f32_bwd(dh1, x, w[0], need_dx=False)
    got = dict(out=out, **{"d " + n: grads[n] for n in NAMES})
    for n in got:
        e1, e2 = rel_err(got[n], comp[n]), rel_err(comp[n], got[n])
        print(f"{shape} {n}: new vs composed {e1:.3e}, composed vs new {e2:.3e}")
        assert e1 < GATE and e2 < GATE, (shape, n, e1, e2)


# ---- training, evaluation, checkpoints -------------------------------------------------------------------------------------------------
def two_tower_model(dev):
    from clibd_amd.model import MLPEncoder, SimpleCLIP

    g = _golden()
    i, h, o = g["dims"]
    model = SimpleCLIP(MLPEncoder(i, h, o), MLPEncoder(i, h, o), None)
    model.load_state_dict(g["trajectory"]["init"])
    return model.to(dev)


def test_trainer_trajectory_matches_the_reference(dev):
    """`Trainer` (all_gather=False: ContrastiveLoss; the temperature fixed at 0.07 as the fixture's loop passes 1 / 0.07; FusedAdamW at
    torch.optim.AdamW's defaults) on the fixture's two towers and batch, 20 steps: every loss within 2e-4 |ref| + 1e-3 of the reference's
    (the replay gate of tests/test_method_linear_gpu.py), every final weight tensor at rel_err < 1e-3."""
    from clibd_amd.train import Trainer

    t = _golden()["trajectory"]
    model = two_tower_model(dev)
    model.train()
    tr = Trainer(model, lr=t["lr"], all_gather=False, fix_temperature=0.07)
    assert tr.optimizer.flat_g.numel() >= sum(p.numel() for n, p in model.named_parameters() if n != "logit_scale")
    image, dna, labels = t["image"].to(dev), t["dna"].to(dev), t["labels"].to(dev)
    losses = torch.stack([tr.step(image, dna, None, labels) for _ in range(len(t["losses"]))]).double().cpu()
    ref = t["losses"]
    worst = ((losses - ref).abs() / (2e-4 * ref.abs() + 1e-3)).max().item()
    print(f"trajectory: losses {losses[0]:.5f} -> {losses[-1]:.5f} (reference {ref[0]:.5f} -> {ref[-1]:.5f}), worst |diff| / gate {worst:.3e}")
    assert all(loss_close(a, b) for a, b in zip(losses.tolist(), ref.tolist())), worst
    assert losses[-1] < 0.5 * losses[0]
    sd = model.state_dict()
    for k, v in t["final"].items():
        e = rel_err(sd[k], v)
        print(f"trajectory final {k}: rel_err {e:.3e}")
        assert e < 1e-3, (k, e)


def test_eval_loop_passes_float_features_through(dev):
    """get_feature_and_label over the reference's 7-tuples with float feature rows in the image and DNA slots returns the normalised
    embeddings the reference's model gave for them"""
    from clibd_amd import eval as E

    t = _golden()["trajectory"]
    model = two_tower_model(dev)
    n = t["image"].shape[0]
    batches = []
    for s in range(0, n, 24):                                              # 24, 24, 16 rows
        e = min(n, s + 24)
        ids = torch.zeros(e - s, 4, dtype=torch.long)
        batches.append(([f"p{r}" for r in range(s, e)], t["image"][s:e], t["dna"][s:e], ids, ids, ids,
                        {k: [f"{k}{int(l)}" for l in t["labels"][s:e]] for k in ("order", "family", "genus", "species")}))
    names, img, dna, txt, labels = E.get_feature_and_label(batches, model, dev, as_numpy=False)
    assert names == [f"p{r}" for r in range(n)] and txt is None and len(labels) == n and labels[3]["species"] == "species1"
    for name, got, ref in (("image", img, t["embed_image"]), ("dna", dna, t["embed_dna"])):
        e = rel_err(got, ref)
        print(f"eval {name}: rel_err {e:.3e}")
        assert tuple(got.shape) == tuple(ref.shape) and e < GATE, (name, e)


def test_checkpoints_round_trip_bit_for_bit(dev, tmp_path):
    from clibd_amd.checkpoint import export_reference_state_dict, load_reference_checkpoint, load_training_state, save_training_state
    from clibd_amd.train import Trainer

    t = _golden()["trajectory"]
    model = two_tower_model(dev)
    tr = Trainer(model, lr=t["lr"], all_gather=False, fix_temperature=0.07)
    model.train()
    tr.step(t["image"].to(dev), t["dna"].to(dev), None, t["labels"].to(dev))
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert list(sd) == list(t["init"]) and not torch.equal(sd["image_encoder.encoder.0.weight"], t["init"]["image_encoder.encoder.0.weight"])
    save_training_state(str(tmp_path / "state.pth"), model, tr.optimizer, epoch=1)
    torch.save({"module." + k: v for k, v in export_reference_state_dict(model).items()}, tmp_path / "last.pth")     # as DDP would write it
    other = two_tower_model(dev)
    load_training_state(str(tmp_path / "state.pth"), other)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in other.state_dict().items())
    third = two_tower_model(dev)
    load_reference_checkpoint(third, str(tmp_path / "last.pth"))
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in third.state_dict().items())
    x = t["image"].to(dev)
    with torch.no_grad():
        assert torch.equal(third.image_encoder(x), model.image_encoder(x))
    state = torch.load(tmp_path / "state.pth", weights_only=False)
    assert state["deterministic"] is True and state["numerics"]["dna_encoder"] == {"forward": "fp32-grade (split bf16)"}


def test_model_switches_do_not_raise_on_feature_towers(dev):
    model = two_tower_model(dev)
    assert model.set_deterministic(True) is model and model.enable_fp8_dgrad() is model and model.set_numerics(residual_grad="fp32") is model
    assert model.enable_fp8_forward(enabled=False) is model and model.deterministic()
    assert model.numerics() == {n: {"forward": "fp32-grade (split bf16)"} for n in ("image_encoder", "dna_encoder")}
    t = _golden()["trajectory"]
    img, dna, txt, scale, bias = model(t["image"].to(dev), t["dna"].to(dev), None)
    model.join_streams()
    assert txt is None and bias is None and rel_err(img, t["embed_image"]) < GATE and rel_err(dna, t["embed_dna"]) < GATE
