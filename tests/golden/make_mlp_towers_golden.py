"""Generate tests/golden/mlp_towers_golden.pt by IMPORTING THE REFERENCE's feature towers (authoring container only, CPU):

    python tests/golden/make_mlp_towers_golden.py

bioscanclip.model.mlp.{MLPEncoder, MLPVersionCLIP} and bioscanclip.model.simple_clip.SimpleCLIP are plain torch; ContrastiveLoss comes in
the way make_golden.py imports it (same stubs for the reference's unused third-party imports).  Only DATA is written: key lists, seeded
weights, inputs, fp64 results and a 20-step fp32 AdamW trajectory; no reference source is copied.

  keys         state-dict key lists of MLPEncoder, MLPVersionCLIP and SimpleCLIP(MLPEncoder, MLPEncoder, None)
  init         the state dicts those constructors draw under torch.manual_seed(SEED), at the small INIT_DIMS (torch's default
               initialisation depends on the shapes only through fan-in: small tensors check the draw order as well as large ones)
  tower        one MLPEncoder (DIMS): weights (hidden biases moved so that no pre-activation is within 1e-4 of 0, see
               keep_preactivations_off_zero), x, an upstream gradient dout; fp64 out, the gradient of every parameter and
               dh2, dh1 = the gradients that reach the pre-activations of layers 2 and 1 (what the two dgrad launches write)
  trajectory   SimpleCLIP of two MLPEncoders, F.normalize (inside SimpleCLIP.forward), ContrastiveLoss at logit scale 1 / 0.07,
               torch.optim.AdamW(lr=1e-3): initial weights, the batch, 20 losses, final weights, the initial normalised embeddings
"""
import importlib.util
import os

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mlp_towers_golden.pt")
SEED = 1234
DIMS = (96, 64, 48)       # input, hidden, output
INIT_DIMS = (20, 32, 16)
PAIRS, STEPS, LR = 64, 20, 1e-3


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    ref = _make_golden().import_reference()
    from bioscanclip.model import mlp

    return mlp, ref["simple_clip"], ref["loss_func"]


MARGIN, REACH = 1e-4, 0.05


def keep_preactivations_off_zero(sd, x, margin=MARGIN, reach=REACH):
    """A copy of `sd` whose hidden biases (layers 1 and 2) moved by at most `reach`, each to the point between two zero crossings of its
    unit that keeps every pre-activation of the batch `x` farthest from 0; asserts that `margin` is kept (in fp64, with the fp32 bias).
    Why: a pre-activation within the arithmetic's rounding of 0 (fp32-grade: ~1e-6 here) may take the other side of the ReLU than the
    fp64 reference, and ONE flipped mask bit moves a whole element of dh, i.e. 1 / sqrt(elements) of its norm — 6e-3 at 77 x 64, far above
    a 1e-4 gate, in ANY correct implementation.  With 1e-4 of room the masks of the reference and of an fp32-grade forward are the same."""
    sd = {k: v.clone() for k, v in sd.items()}
    a = x.double()
    for j in (0, 2):
        z = a @ sd[f"encoder.{j}.weight"].double().T
        bias = sd[f"encoder.{j}.bias"].double().clone()
        for u in range(z.shape[1]):
            cross = torch.sort(-z[:, u]).values                            # the bias values at which a row of this unit crosses 0
            cand = torch.cat([bias[u : u + 1], bias[u : u + 1] - reach, bias[u : u + 1] + reach, (cross[1:] + cross[:-1]) / 2])
            cand = cand[(cand - bias[u]).abs() <= reach]
            room = (z[:, u, None] + cand[None, :]).abs().min(0).values
            bias[u] = cand[room.argmax()]
        sd[f"encoder.{j}.bias"] = bias.float()
        pre = z + sd[f"encoder.{j}.bias"].double()
        assert pre.abs().min() > margin, (j, float(pre.abs().min()))
        a = torch.relu(pre)
    return sd


def tower_fp64(sd, x, dout):
    """fp64 forward and backward of Linear, ReLU, Linear, ReLU, Linear written out (torch's ReLU backward: h > 0)"""
    w1, b1, w2, b2, w3, b3 = (sd[f"encoder.{i}.{n}"].double() for i in (0, 2, 4) for n in ("weight", "bias"))
    x, dout = x.double(), dout.double()
    h1 = torch.relu(x @ w1.T + b1)
    h2 = torch.relu(h1 @ w2.T + b2)
    out = h2 @ w3.T + b3
    dh2 = (dout @ w3) * (h2 > 0)
    dh1 = (dh2 @ w2) * (h1 > 0)
    grads = {"encoder.4.weight": dout.T @ h2, "encoder.4.bias": dout.sum(0), "encoder.2.weight": dh2.T @ h1, "encoder.2.bias": dh2.sum(0),
             "encoder.0.weight": dh1.T @ x, "encoder.0.bias": dh1.sum(0)}
    return dict(out=out, h1=h1, h2=h2, dh2=dh2, dh1=dh1, grads=grads)


def main():
    mlp, simple_clip, lf = import_reference()
    i, h, o = DIMS
    out = {"seed": SEED, "dims": DIMS}

    def two_towers(i=i, h=h, o=o):
        return simple_clip.SimpleCLIP(image_encoder=mlp.MLPEncoder(input_dim=i, hidden_dim=h, output_dim=o),
                                      dna_encoder=mlp.MLPEncoder(input_dim=i, hidden_dim=h, output_dim=o), language_encoder=None)

    si, sh, so = INIT_DIMS
    made = {"MLPEncoder": lambda: mlp.MLPEncoder(si, sh, so), "MLPVersionCLIP": lambda: mlp.MLPVersionCLIP(si, si + 16, sh, so),
            "SimpleCLIP": lambda: two_towers(si, sh, so)}
    out["keys"], out["init"], out["init_dims"] = {}, {}, INIT_DIMS
    for name, make in made.items():
        torch.manual_seed(SEED)
        sd = make().state_dict()
        out["keys"][name] = list(sd.keys())
        out["init"][name] = {k: v.clone() for k, v in sd.items()}

    # ---- one tower against fp64, and the module itself as a cross-check of the written-out backward
    g = torch.Generator().manual_seed(SEED)
    torch.manual_seed(SEED + 1)
    enc = mlp.MLPEncoder(i, h, o)
    x, dout = torch.randn(PAIRS + 13, i, generator=g), torch.randn(PAIRS + 13, o, generator=g)
    sd = keep_preactivations_off_zero(enc.state_dict(), x)
    t = tower_fp64(sd, x, dout)
    enc64 = mlp.MLPEncoder(i, h, o).double()
    enc64.load_state_dict({k: v.double() for k, v in sd.items()})
    (enc64(x.double()) * dout.double()).sum().backward()
    for n, p in enc64.named_parameters():
        assert torch.allclose(p.grad, t["grads"][n], rtol=1e-12, atol=1e-12), n
    t.pop("h1"), t.pop("h2")
    out["tower"] = dict(state_dict=sd, x=x, dout=dout, **t)

    # ---- the 20-step trajectory (fp32, the reference's own modules and torch's AdamW)
    torch.manual_seed(SEED + 2)
    model = two_towers()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    image, dna = torch.randn(PAIRS, i, generator=g), torch.randn(PAIRS, i, generator=g)
    labels = torch.arange(PAIRS) // 2          # pairs of equal labels: the label matrix has off-diagonal positives
    crit = lf.ContrastiveLoss(criterion=nn.CrossEntropyLoss(), logit_scale=1 / 0.07)
    params = list(model.image_encoder.parameters()) + list(model.dna_encoder.parameters())
    opt = torch.optim.AdamW(params, lr=LR)
    with torch.no_grad():
        e_img, e_dna = model(image, dna, None)[:2]
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        img_o, dna_o, txt_o, _scale, _bias = model(image, dna, None)
        loss = crit(img_o, dna_o, txt_o, labels, 1 / 0.07)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    out["trajectory"] = dict(init=init, image=image, dna=dna, labels=labels, lr=LR, losses=torch.tensor(losses, dtype=torch.float64),
                             final={k: v.clone() for k, v in model.state_dict().items()}, embed_image=e_img.clone(), embed_dna=e_dna.clone())
    torch.save(out, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); losses {losses[0]:.4f} -> {losses[-1]:.4f}")


if __name__ == "__main__":
    main()
