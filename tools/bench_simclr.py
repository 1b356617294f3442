"""SimCLR pre-training step on the MI355X: ms per step and images/s at b = 256 (512 images) and b = 500 (the reference's batch, 1000
images), with the loss (forward + backward) and the Adam step as separate device times, and — for comparison at the same N — the
existing contrastive pair clibd_softce_rows_fwd + bwd at Nx = N = 2b, D = 1024 (K9 needs D % 64 == 0).

    python tools/bench_simclr.py [--batches 256 500] [--model vit_base_patch16_224] [--windows 5]

Method: every shape is warmed up first; each figure is the median over `--windows` windows of device-event time, a window holding
enough repetitions to last well above the event resolution (3 steps, or 20 loss / optimizer calls).  Records, not gates.
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, windows):
    """median over `windows` of (device time of `reps` calls) / reps, in ms; also the min and max window"""
    out = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) / reps)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 500])
    ap.add_argument("--model", default="vit_base_patch16_224")
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simclr needs an MI355X (no CPU path)")
    from clibd_amd import ops
    from clibd_amd.build import csrc_hash
    from clibd_amd.optim import FusedAdam
    from clibd_amd.simclr import SimCLR, load_vit_for_simclr_training

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mc = types.SimpleNamespace(temperature=0.07, n_views=2, epochs=1, model_output_name="bench", image=types.SimpleNamespace(pre_train_model=a.model))
    args = types.SimpleNamespace(model_config=mc, project_root_path=".")
    model = load_vit_for_simclr_training(args, device=dev)
    opt = FusedAdam(model.parameters(), lr=3e-4, weight_decay=1e-4)
    sim = SimCLR(model=model, optimizer=opt, scheduler=None, device=dev, args=args)
    print(json.dumps(dict(what="setup", model=a.model, parameters=int(opt.flat_p.numel()), csrc=csrc_hash(), device=torch.cuda.get_device_name(0))), flush=True)
    for b in a.batches:
        N = 2 * b
        g = torch.Generator(device=dev).manual_seed(b)
        v1, v2 = torch.rand(b, 3, 224, 224, device=dev, generator=g), torch.rand(b, 3, 224, 224, device=dev, generator=g)
        for _ in range(2):
            loss = sim.train_step(v1, v2)
        torch.cuda.synchronize()
        step = timed(lambda: sim.train_step(v1, v2), 3, a.windows)
        # the loss alone on features of the step's shape
        f = torch.randn(N, 1000, device=dev, generator=g) * 3
        ws, lo, df, t1 = ops.ntxent_workspace(N, 1000, dev), torch.empty(1, device=dev), torch.empty(N, 1000, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

        def ntx_fwd():
            ops.ntxent_fwd(f, 1 / 0.07, lo, ws, t1)

        def ntx_pair():
            ops.ntxent_fwd(f, 1 / 0.07, lo, ws, t1)
            ops.ntxent_bwd(f, 1 / 0.07, df, ws)

        ntx_pair()
        ntx_f, ntx = timed(ntx_fwd, 20, a.windows), timed(ntx_pair, 20, a.windows)
        # K9 at the same N (normalised inputs, identity labels), D = 1024
        x = torch.nn.functional.normalize(torch.randn(N, 1024, device=dev, generator=g), dim=1).contiguous()
        labels, scale = torch.arange(N, device=dev), torch.tensor([1 / 0.07], device=dev)
        kws, ksum, dx, dy = ops.softce_workspace(N, N, 1024, dev), torch.zeros(1, device=dev), torch.zeros(N, 1024, device=dev), torch.zeros(N, 1024, device=dev)

        def k9_pair():
            ops.softce_rows_fwd(x, x, labels, 0, scale, ksum, kws)
            ops.softce_rows_bwd(labels, N, N, 1024, 0, scale, 1.0 / N, dx, dy, None, kws)

        k9_pair()
        k9 = timed(k9_pair, 20, a.windows)
        adam = timed(opt.step, 20, a.windows)
        print(json.dumps(dict(what="simclr_step", b=b, images=N, loss=float(loss), ms_per_step=step, images_per_s=N / step["median_ms"] * 1e3,
                              ntxent_fwd_ms=ntx_f, ntxent_fwd_bwd_ms=ntx, k9_softce_fwd_bwd_D1024_ms=k9, adam_step_ms=adam,
                              ntxent_workspace_MiB=ws.numel() / 2 ** 20, k9_workspace_MiB=kws.numel() / 2 ** 20)), flush=True)
        del v1, v2, f, ws, kws, x, dx, dy, df
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
