"""Time of the pre-extracted-feature towers (clibd_amd.towers.MLPTower, include/clibd_hip_mlp.h) at a workload shape.

    python tools/bench_mlp_towers.py [--batch 2048] [--input-dim 768] [--hidden-dim 512] [--output-dim 512] [--out profiles/mlp_towers.log]

B = 2048, dims 768 / 512 / 512 (MLPVersionCLIP's defaults with a ViT-B-wide input).  After a warm-up it times, as medians of 5 windows of
device-event time,
  (a) one tower forward (three clibd_mlp_linear_fwd launches),
  (b) forward + backward (plus three wgrad and two dgrad launches, gradients accumulated into a flat buffer as under the trainer),
  (c) a whole two-tower `Trainer.step` (both towers, L2 norms, ContrastiveLoss, fused AdamW),
and, for the same (a) and (b), the tower COMPOSED from the linear-probe head's ops.linear_f32_fwd / linear_f32_bwd plus torch's ReLU and
mask multiplies: the yardstick (about sixty launches per tower step against eight), on the same weights and inputs.  Each kernel role is
timed alone at every layer shape as well.  Records, not gates: there is no earlier implementation of the feature.
Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_ms(fn, iters=20, windows=5):
    import torch

    out = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--input-dim", type=int, default=768)
    ap.add_argument("--hidden-dim", type=int, default=512)
    ap.add_argument("--output-dim", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from clibd_amd import ops
    from clibd_amd.build import csrc_hash
    from clibd_amd.model import MLPEncoder, SimpleCLIP
    from clibd_amd.train import Trainer

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, i, h, o = a.batch, a.input_dim, a.hidden_dim, a.output_dim
    enc = MLPEncoder(i, h, o).to(dev)
    x, dout = torch.randn(B, i, device=dev), torch.randn(B, o, device=dev)
    tw = enc.tower()
    params = tw.trainable_params()
    tw.grad_sink = {id(p): torch.zeros_like(p) for p in params}      # as under the trainer: gradients accumulate in place

    def fwd():
        with torch.no_grad():
            return enc(x)

    def fwd_bwd():
        enc(x).backward(dout)

    w = [enc.encoder[j].weight.detach() for j in (0, 2, 4)]
    b = [enc.encoder[j].bias.detach() for j in (0, 2, 4)]

    def composed_fwd():
        h1 = torch.relu(ops.linear_f32_fwd(x, w[0], b[0]))
        h2 = torch.relu(ops.linear_f32_fwd(h1, w[1], b[1]))
        return h1, h2, ops.linear_f32_fwd(h2, w[2], b[2])

    def composed_fwd_bwd():
        h1, h2, _ = composed_fwd()
        dh2, _, _ = ops.linear_f32_bwd(dout, h2, w[2])
        dh1, _, _ = ops.linear_f32_bwd(dh2 * (h2 > 0), h1, w[1])
        ops.linear_f32_bwd(dh1 * (h1 > 0), x, w[0], need_dx=False)

    for fn in (fwd, fwd_bwd, composed_fwd, composed_fwd_bwd):
        fn()
    torch.cuda.synchronize()
    rec = {"tool": "bench_mlp_towers", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "batch": B, "dims": [i, h, o],
           "tower_fwd_device_ms": round(device_ms(fwd), 4), "tower_fwd_bwd_device_ms": round(device_ms(fwd_bwd), 4),
           "composed_fwd_device_ms": round(device_ms(composed_fwd), 4), "composed_fwd_bwd_device_ms": round(device_ms(composed_fwd_bwd), 4)}
    rec["composed_over_new_fwd"] = round(rec["composed_fwd_device_ms"] / rec["tower_fwd_device_ms"], 3)
    rec["composed_over_new_fwd_bwd"] = round(rec["composed_fwd_bwd_device_ms"] / rec["tower_fwd_bwd_device_ms"], 3)

    # ---- each role alone, per layer shape (K -> N)
    per = {}
    for name, (K, N) in (("layer1", (i, h)), ("layer2", (h, h)), ("layer3", (h, o))):
        xs, dy = torch.randn(B, K, device=dev), torch.randn(B, N, device=dev)
        ws, bs, hs = torch.randn(N, K, device=dev) * 0.05, torch.zeros(N, device=dev), torch.relu(torch.randn(B, K, device=dev))
        dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        per[name] = {"K": K, "N": N,
                     "fwd_ms": round(device_ms(lambda: ops.mlp_linear_fwd(xs, ws, bs, relu=True)), 4),
                     "dgrad_ms": round(device_ms(lambda: ops.mlp_linear_dgrad(dy, ws, hs)), 4),
                     "wgrad_ms": round(device_ms(lambda: ops.mlp_linear_wgrad(dy, xs, dw, db, accumulate=True)), 4)}
    rec["per_kernel"] = per

    # ---- a whole two-tower training step
    model = SimpleCLIP(MLPEncoder(i, h, o), MLPEncoder(i, h, o), None).to(dev)
    model.train()
    tr = Trainer(model, lr=1e-3, all_gather=False, fix_temperature=0.07)
    img, dna, labels = torch.randn(B, i, device=dev), torch.randn(B, i, device=dev), torch.arange(B, device=dev)
    for _ in range(3):
        tr.step(img, dna, None, labels)
    torch.cuda.synchronize()
    rec["trainer_step_device_ms"] = round(device_ms(lambda: tr.step(img, dna, None, labels), iters=10), 4)

    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
