"""Time of the attention rollout (clibd_amd.rollout) at the ViT-B/16 shape of the reference's figures.

    python tools/bench_rollout.py [--batch 64] [--layers 5] [--fusion max] [--ratio 0.9] [--out profiles/rollout.log]

B = 64 images, S = 197, 12 heads, five layers (the ViT window [1:-6]), `max`, discard ratio 0.9.  After a warm-up, device-event medians
(five windows of 200 back-to-back repeats for the kernels, of 20 for the torch restatement, the forward and the whole call) of
  1. clibd_attn_fused_maps over the five layers' packed qkv (N(0, 1) bf16), next to what it reads and writes;
  2. clibd_rollout_discard on the [5, 64] maps (in place: each repeat restores the maps first, and the restore is timed alone beside it);
  3. clibd_rollout_chain;
  4. the whole call `attention_rollout(encoder, images)` on a randomly initialised ViT-B/16 encoder, beside the encoder's plain eval
     forward (the recording forward is part of the call).
Beside them a plain-torch-on-device restatement of 1-3 that materialises P ([B, heads, S, S] fp32 per layer), selects with torch.topk and
chains with batched matrix products, as the reference's loop does per image.  Records, not gates: there is no parent to compare with.
Prints one JSON line (and appends it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_ms(fn, iters=200, windows=5):
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


def torch_rollout(qkvs, B, S, heads, fusion, k):
    """the reference's arithmetic in plain torch on the device, batched over images (each image on its own, as clibd_amd.rollout treats a batch)"""
    import torch

    result = torch.eye(S, device=qkvs[0].device).expand(B, S, S)
    eye = torch.eye(S, device=qkvs[0].device)
    for qkv in qkvs:
        x = qkv.view(B, S, 3, heads, 64).float()
        q, kk = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
        P = torch.softmax((q @ kk.transpose(-1, -2)) * 0.125, dim=-1)
        F = P.mean(1) if fusion == "mean" else (P.max(1)[0] if fusion == "max" else P.min(1)[0])
        flat = F.reshape(B, -1)
        _, idx = flat.topk(k, -1, False)
        keep00 = flat[:, 0].clone()
        flat.scatter_(1, idx, 0.0)
        flat[:, 0] = keep00
        a = (F + eye) / 2
        a = a / a.sum(dim=-1)[:, None, :]
        result = a @ result
    mask = result[:, 0, 1:]
    return mask / mask.max(dim=-1, keepdim=True)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--fusion", default="max")
    ap.add_argument("--ratio", type=float, default=0.9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from clibd_amd import ops
    from clibd_amd import rollout as R
    from clibd_amd.build import csrc_hash
    from clibd_amd.model.image_encoder import CLIBDImageEncoder, create_vit

    dev = torch.device("cuda:0")
    B, S, heads, L = a.batch, 197, 12, a.layers
    ld = ops.rollout_ld(S)
    k = R.discard_count(S, a.ratio)
    code = R.FUSIONS[a.fusion]
    gen = torch.Generator().manual_seed(0)
    qkvs = [torch.randn(B * S, 3 * 64 * heads, generator=gen).to(torch.bfloat16).to(dev) for _ in range(L)]
    maps = torch.empty((L, B, S, ld), dtype=torch.float32, device=dev)

    def fused():
        for l in range(L):
            ops.attn_fused_maps(qkvs[l], B, S, heads, code, out=maps[l])

    fused()
    t_fused = device_ms(fused)
    pristine = maps.clone()
    work = maps.clone()

    def restore():
        work.copy_(pristine)

    def restore_discard():
        work.copy_(pristine)
        ops.rollout_discard_(work, S, k)

    restore_discard()
    t_restore, t_restore_discard = device_ms(restore), device_ms(restore_discard)
    ops.rollout_chain(work, S)
    t_chain = device_ms(lambda: ops.rollout_chain(work, S))
    mask = ops.rollout_chain(work, S)

    ref = torch_rollout(qkvs, B, S, heads, a.fusion, k)
    t_torch = device_ms(lambda: torch_rollout(qkvs, B, S, heads, a.fusion, k), iters=20, windows=5)
    diff = float((mask - ref).abs().max())

    torch.manual_seed(0)
    enc = CLIBDImageEncoder(create_vit("vit_base_patch16_224", num_classes=0), r=4, num_classes=768).to(dev).eval()
    img = torch.rand(B, 3, 224, 224, generator=gen).to(dev)
    with torch.no_grad():
        enc(img)
    R.attention_rollout(enc, img, a.fusion, a.ratio)

    def forward():
        with torch.no_grad():
            enc(img)

    t_forward = device_ms(forward, iters=20, windows=5)
    t_call = device_ms(lambda: R.attention_rollout(enc, img, a.fusion, a.ratio), iters=20, windows=5)

    rec = {"tool": "bench_rollout", "csrc_hash": csrc_hash(), "gpu": torch.cuda.get_device_name(0), "batch": B, "S": S, "heads": heads, "layers": L,
           "fusion": a.fusion, "ratio": a.ratio, "k": k,
           "fused_maps_device_ms": round(t_fused, 4), "fused_maps_read_mb": round(L * B * S * 2 * 64 * heads * 2 / 1e6, 1),
           "fused_maps_write_mb": round(L * B * S * ld * 4 / 1e6, 1), "per_head_maps_would_write_mb": round(L * B * heads * S * S * 4 / 1e6, 1),
           "restore_device_ms": round(t_restore, 4), "restore_plus_discard_device_ms": round(t_restore_discard, 4),
           "discard_device_ms": round(t_restore_discard - t_restore, 4), "chain_device_ms": round(t_chain, 4),
           "three_kernels_device_ms": round(t_fused + t_restore_discard - t_restore + t_chain, 4),
           "torch_on_device_restatement_ms": round(t_torch, 4), "max_abs_mask_difference_to_it": diff,
           "encoder_eval_forward_ms": round(t_forward, 3), "attention_rollout_whole_call_ms": round(t_call, 3)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
