"""The SimCLR view generator on the MI355X against the host pipeline it replaces.

    python tools/bench_simclr_views.py [--batches 256 500] [--model vit_base_patch16_224] [--windows 5] [--host-views 48] [--no-step]

Three records per batch size b (n = 2b views of b distinct 256 x 341 images, records drawn by the sampler):
  * the device time of clibd_simclr_views_u8 (ops.simclr_views with a reused workspace), views/s, and the bytes it has to move
    (the uint8 source once, the fp32 pre-jitter image written and read, the fp32 output written) over that time;
  * the SimCLR step fed from the packed batch (resident on the device, as the prefetcher leaves it) against the step fed from two
    resident view tensors, in alternating windows;
and one host record: views/s of the pipeline the reference runs in its DataLoader workers (torchvision's PIL backend restated with PIL
and torch: crop().resize(BILINEAR), ImageEnhance, the uint8 hue shift, convert("L"), the 21 x 21 depth-wise blur on the uint8 tensor),
on one thread and on `--threads` threads of a pool (PIL and torch release the interpreter lock in their kernels; torch's own pool is
held at one thread per worker, as in a DataLoader worker).  The host record is taken only when PIL is installed.

Method (tools/bench_simclr.py): every shape is warmed up first; each device figure is the median over `--windows` windows of
device-event time, a window holding enough repetitions to last well above the event resolution.  Records, not gates.
"""
import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 256, 341


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


def timed_alternating(fns, reps, windows):
    """the same for several variants, their windows interleaved so that drift of the machine hits all alike"""
    out = [[] for _ in fns]
    for _ in range(windows):
        for k, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            e.synchronize()
            out[k].append(s.elapsed_time(e) / reps)
    return [dict(median_ms=statistics.median(o), min_ms=min(o), max_ms=max(o)) for o in out]


def images(b, seed=0):
    """b distinct H x W uint8 images: smooth colour gradients plus noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(b):
        base = 127 + 100 * np.sin(yy[..., None] * (0.03 + 0.0001 * i) + xx[..., None] * 0.03 + 2.1 * np.arange(3) + i)
        out.append(np.clip(base + rng.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8))
    return out


# ---- the host pipeline: torchvision's PIL backend, restated -----------------------------------------------------------------------
def host_view(im, v):
    from PIL import Image, ImageEnhance

    im = im.crop((v["left"], v["top"], v["left"] + v["w"], v["top"] + v["h"])).resize((224, 224), Image.BILINEAR)
    if v["hflip"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if v["jitter"]:
        for op in v["ops"]:
            if op == 0:
                im = ImageEnhance.Brightness(im).enhance(v["brightness"])
            elif op == 1:
                im = ImageEnhance.Contrast(im).enhance(v["contrast"])
            elif op == 2:
                im = ImageEnhance.Color(im).enhance(v["saturation"])
            else:
                h, s, val = im.convert("HSV").split()
                nh = ((np.array(h, dtype=np.int64) + int(v["hue"] * 255)) % 256).astype(np.uint8)
                im = Image.merge("HSV", (Image.fromarray(nh, "L"), s, val)).convert("RGB")
    if v["gray"]:
        g = np.array(im.convert("L"))
        im = Image.fromarray(np.dstack([g, g, g]), "RGB")
    x = torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().to(torch.float32)[None]
    k = torch.linspace(-10, 10, 21)
    pdf = torch.exp(-0.5 * (k / v["sigma"]) ** 2)
    k1 = pdf / pdf.sum()
    k2 = (k1[:, None] @ k1[None, :]).expand(3, 1, 21, 21)
    x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (10, 10, 10, 10), mode="reflect"), k2, groups=3)
    return x.round().to(torch.uint8)[0].to(torch.float32).div(255)          # GaussianBlur's cast back, then ToTensor


def host_rates(n_views, threads):
    from PIL import Image

    from clibd_amd import simclr_views as V

    imgs = [Image.fromarray(a) for a in images(4, seed=1)]
    p = V.params_from_uniforms([(H, W)] * (n_views // 2), V.draw_view_uniforms(n_views // 2, torch.Generator().manual_seed(0)))
    views = [dict(top=int(p["top"][r]), left=int(p["left"][r]), h=int(p["h"][r]), w=int(p["w"][r]), hflip=bool(p["hflip"][r]), jitter=bool(p["jitter"][r]),
                  gray=bool(p["gray"][r]), ops=tuple(int(o) for o in p["ops"][r]), brightness=float(p["brightness"][r]), contrast=float(p["contrast"][r]),
                  saturation=float(p["saturation"][r]), hue=float(p["hue"][r]), sigma=float(p["sigma"][r])) for r in range(n_views)]
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        host_view(imgs[0], views[0])                                   # warm-up
        t = time.perf_counter()
        for r, v in enumerate(views):
            host_view(imgs[r % 4], v)
        one = n_views / (time.perf_counter() - t)
        with cf.ThreadPoolExecutor(max_workers=threads) as ex:
            list(ex.map(lambda rv: host_view(imgs[rv[0] % 4], rv[1]), enumerate(views[:threads])))
            t = time.perf_counter()
            list(ex.map(lambda rv: host_view(imgs[rv[0] % 4], rv[1]), [(r, v) for _ in range(4) for r, v in enumerate(views)]))
            many = 4 * n_views / (time.perf_counter() - t)
    finally:
        torch.set_num_threads(before)
    return dict(what="host_pil_path", views=n_views, image=[H, W], views_per_s_one_thread=one, ms_per_view_one_thread=1e3 / one, threads=threads,
                views_per_s_threads=many, cpus=len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 500])
    ap.add_argument("--model", default="vit_base_patch16_224")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-views", type=int, default=48)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-step", action="store_true", help="time the transform only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simclr_views needs an MI355X (no CPU path)")
    from clibd_amd import _lib, ops
    from clibd_amd import simclr_views as V
    from clibd_amd.build import csrc_hash

    try:
        import PIL  # noqa: F401
    except ImportError:
        print(json.dumps(dict(what="host_pil_path", skipped="PIL is not installed")), flush=True)
    else:
        print(json.dumps(host_rates(a.host_views, a.threads)), flush=True)

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(json.dumps(dict(what="setup", model=None if a.no_step else a.model, csrc=csrc_hash(), device=torch.cuda.get_device_name(0))), flush=True)
    sim = None
    if not a.no_step:
        from clibd_amd.optim import FusedAdam
        from clibd_amd.simclr import SimCLR, load_vit_for_simclr_training

        mc = types.SimpleNamespace(temperature=0.07, n_views=2, epochs=1, model_output_name="bench", image=types.SimpleNamespace(pre_train_model=a.model))
        args = types.SimpleNamespace(model_config=mc, project_root_path=".")
        model = load_vit_for_simclr_training(args, device=dev)
        sim = SimCLR(model=model, optimizer=FusedAdam(model.parameters(), lr=3e-4, weight_decay=1e-4), scheduler=None, device=dev, args=args)
    for b in a.batches:
        n = 2 * b
        imgs = images(b, seed=b)
        sizes = np.array([[H, W]] * b, dtype=np.int64)
        data = torch.from_numpy(np.concatenate([x.reshape(-1) for x in imgs])).to(dev)
        xf = V.sample_view_params(sizes, torch.Generator().manual_seed(b)).to(dev)
        ws = torch.empty((int(_lib.load().clibd_simclr_views_workspace_bytes(n)),), dtype=torch.uint8, device=dev)
        for _ in range(3):
            views = ops.simclr_views(data, xf, ws)
        torch.cuda.synchronize()
        t = timed(lambda: ops.simclr_views(data, xf, ws), 10, a.windows)
        image_bytes = 3 * 224 * 224 * 4
        moved = data.numel() + n * 3 * image_bytes                              # source once; pre-jitter image written, read; output written
        rec = dict(what="simclr_views", b=b, views=n, transform_ms=t, views_per_s=n / t["median_ms"] * 1e3, source_MB=data.numel() / 1e6,
                   two_fp32_views_MB=n * image_bytes / 1e6, workspace_MiB=ws.numel() / 2 ** 20, bytes_moved_GB=moved / 1e9,
                   moved_GB_per_s=moved / 1e9 / (t["median_ms"] * 1e-3))
        if sim is not None:
            v1, v2 = views[:b].clone(), views[b:].clone()
            packed = {"data": data, "offsets": None, "xforms": xf}
            for _ in range(2):
                sim.train_step(v1, v2)
                loss = sim.train_step(packed)
            torch.cuda.synchronize()
            resident, fed = timed_alternating([lambda: sim.train_step(v1, v2), lambda: sim.train_step(packed)], 3, a.windows)
            rec.update(loss=float(loss), step_from_tensors_ms=resident, step_from_packed_ms=fed,
                       packed_minus_tensors_ms=fed["median_ms"] - resident["median_ms"], transform_share_of_step=t["median_ms"] / resident["median_ms"],
                       images_per_s_from_packed=n / fed["median_ms"] * 1e3)
            del v1, v2
        print(json.dumps(rec), flush=True)
        del data, xf, ws, views
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
