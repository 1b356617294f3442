"""The two SimCLR views of every image on the device: the host decodes JPEG / PNG bytes once per image, packs the uint8 pixels and draws
the random parameters of both views; the transform chain of the reference's `get_simclr_pipeline_transform` (util/dataset.py:314-325)
runs as HIP (clibd_simclr_views_u8, csrc/views.hip):

    RandomResizedCrop(224) -> RandomHorizontalFlip -> RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], p=0.8) -> RandomGrayscale(0.2)
    -> GaussianBlur(21, sigma=(0.1, 2.0)) -> ToTensor

The arithmetic is torchvision's tensor path for a float image in fp32, with no rounding to uint8 between the stages (the reference
applies the chain to PIL images; DESIGN §3.7 has the measured gap).  The random parameters follow torchvision's samplers in distribution
(not stream for stream: the reference's stream depends on its DataLoader workers): `draw_view_uniforms` draws them in bulk from a seeded
torch.Generator, `params_from_uniforms` turns them into boxes, flips, factors and orders.  A packed batch is a dict of tensors
{"data", "offsets", "xforms"}, so `data.DevicePrefetcher` moves it as it is; the record of sample i's first view is row i of `xforms`
and that of its second view row B + i, the layout `simclr.NTXentLoss` pairs.  `apply` turns the batch into fp32 [2B,3,224,224] on the
device without a host synchronisation; `simclr.SimCLR.train_step` takes the packed batch as it is.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .augment import (ATTEMPTS, _buffers, _check_decode, _pack_device, _packed_offsets, _randint, _sizes, crop_box, decode_images, decode_packed,
                      is_device_packed)

BOX_MAX = 3584                      # crop box side the kernel accepts (224 x 16: at most 34 filter taps per output row / column)
FLAG_HFLIP, FLAG_JITTER, FLAG_GRAY = 1, 2, 4
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
JITTER_P, GRAY_P = 0.8, 0.2
FACTOR, HUE, SIGMA = (0.2, 1.8), (-0.2, 0.2), (0.1, 2.0)   # ColorJitter(0.8, 0.8, 0.8, 0.2): [1 - 0.8, 1 + 0.8] and [-0.2, 0.2]; the blur
# per view: 2 per crop attempt (area, log-ratio); crop top, left; hflip; apply-jitter; 3 for the order of the four operations;
# brightness, contrast, saturation, hue; grayscale; sigma
U_CROP, U_HFLIP, U_JITTER, U_ORDER, U_FACTORS, U_GRAY, U_SIGMA = 0, 2 * ATTEMPTS + 2, 2 * ATTEMPTS + 3, 2 * ATTEMPTS + 4, 2 * ATTEMPTS + 7, 2 * ATTEMPTS + 11, 2 * ATTEMPTS + 12
N_UNIFORMS = 2 * ATTEMPTS + 13
RECORD_INT32 = 16                   # struct clibd_view_xform (include/clibd_hip_views.h): 64 bytes

_RECORD = np.dtype([("offset", "<i8"), ("H0", "<i4"), ("W0", "<i4"), ("top", "<i4"), ("left", "<i4"), ("h", "<i4"), ("w", "<i4"),
                    ("flags", "<i4"), ("order", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue", "<f4"),
                    ("sigma", "<f4"), ("reserved", "<i4")])
assert _RECORD.itemsize == 4 * RECORD_INT32


# ---- random parameters --------------------------------------------------------------------------------------------------------------
def draw_view_uniforms(B: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """float64 [B, 2, N_UNIFORMS] uniforms in [0, 1): everything the two views of B images draw."""
    return torch.rand((B, 2, N_UNIFORMS), dtype=torch.float64, generator=generator)


def op_order(u) -> tuple:
    """torch.randperm(4) in distribution from three uniforms: a Fisher-Yates shuffle of (0, 1, 2, 3)."""
    p = [0, 1, 2, 3]
    for k, i in enumerate((3, 2, 1)):
        j = _randint(float(u[k]), i + 1)
        p[i], p[j] = p[j], p[i]
    return tuple(p)


def pack_order(ops) -> int:
    """the record's `order` word: nibble j holds the id of the operation applied j-th"""
    return sum(int(op) << (4 * j) for j, op in enumerate(ops))


def params_from_uniforms(sizes, uniforms) -> dict:
    """Parameters of both views of every image from their uniforms (pure).  Every array has 2B rows in the record layout: row i is
    sample i's first view, row B + i its second; `image` names the sample."""
    s = _sizes(sizes)
    B = len(s)
    u = np.asarray(uniforms.cpu() if torch.is_tensor(uniforms) else uniforms, dtype=np.float64).reshape(B, 2, N_UNIFORMS)
    u = np.concatenate([u[:, 0], u[:, 1]])                 # [2B, N]
    image = np.concatenate([np.arange(B), np.arange(B)])
    top, left, h, w = (np.empty(2 * B, dtype=np.int64) for _ in range(4))
    ops = np.empty((2 * B, 4), dtype=np.int64)
    for r in range(2 * B):
        H0, W0 = int(s[image[r], 0]), int(s[image[r], 1])
        top[r], left[r], h[r], w[r] = crop_box(H0, W0, u[r, U_CROP:U_HFLIP].tolist())
        ops[r] = op_order(u[r, U_ORDER:U_ORDER + 3])
    f = u[:, U_FACTORS:U_FACTORS + 4]
    return {"image": image, "top": top, "left": left, "h": h, "w": w,
            "hflip": u[:, U_HFLIP] < 0.5,
            "jitter": ~(u[:, U_JITTER] > JITTER_P),        # RandomApply: skipped when p < u
            "ops": ops,
            "brightness": FACTOR[0] + (FACTOR[1] - FACTOR[0]) * f[:, 0],
            "contrast": FACTOR[0] + (FACTOR[1] - FACTOR[0]) * f[:, 1],
            "saturation": FACTOR[0] + (FACTOR[1] - FACTOR[0]) * f[:, 2],
            "hue": HUE[0] + (HUE[1] - HUE[0]) * f[:, 3],
            "gray": u[:, U_GRAY] < GRAY_P,
            "sigma": SIGMA[0] + (SIGMA[1] - SIGMA[0]) * u[:, U_SIGMA]}


# ---- records ------------------------------------------------------------------------------------------------------------------------
def view_records(sizes, params: dict, offsets=None) -> torch.Tensor:
    """int32 [n, 16] records (struct clibd_view_xform) from `params_from_uniforms`'s parameters; `sizes` [B, 2] and `offsets` (byte
    offset of each image in the packed buffer; default: packed back to back, as `decode_images` does) are per IMAGE, `params["image"]`
    names each view's image.  Raises ValueError for what the kernel would answer with a zero image."""
    s = _sizes(sizes)
    B = len(s)
    p = {k: np.asarray(v) for k, v in params.items()}
    image = p["image"].astype(np.int64).reshape(-1)
    n = len(image)
    if n == 0 or (image < 0).any() or (image >= B).any():
        raise ValueError("simclr_views: every view must name one of the images")
    offs = _packed_offsets(s)[:B] if offsets is None else np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)[:B]
    if len(offs) != B or (offs < 0).any():
        raise ValueError("simclr_views: one non-negative byte offset per image")
    if (s > 65535).any():
        raise ValueError("simclr_views: images larger than 65535 pixels on a side are not supported")
    H0, W0 = s[image, 0], s[image, 1]
    for name in ("h", "w"):
        if (p[name] < 1).any() or (p[name] > BOX_MAX).any():
            raise ValueError(f"simclr_views: crop {name} outside [1, {BOX_MAX}]")
    if (p["top"] < 0).any() or (p["left"] < 0).any() or (p["top"] + p["h"] > H0).any() or (p["left"] + p["w"] > W0).any():
        raise ValueError("simclr_views: crop box outside the image")
    ops = p["ops"].astype(np.int64).reshape(n, 4)
    if (np.sort(ops, axis=1) != np.arange(4)).any():
        raise ValueError("simclr_views: the order of the colour operations must be a permutation of (0, 1, 2, 3)")
    rec = np.zeros(n, dtype=_RECORD)
    for name in ("brightness", "contrast", "saturation", "hue", "sigma"):
        rec[name] = p[name]
        if not np.isfinite(rec[name]).all():
            raise ValueError(f"simclr_views: {name} must be finite")
    if (rec["sigma"] < np.float32(SIGMA[0])).any() or (rec["sigma"] > np.float32(SIGMA[1])).any():
        raise ValueError(f"simclr_views: sigma outside [{SIGMA[0]}, {SIGMA[1]}]")
    rec["offset"], rec["H0"], rec["W0"] = offs[image], H0, W0
    rec["top"], rec["left"], rec["h"], rec["w"] = p["top"], p["left"], p["h"], p["w"]
    rec["flags"] = (np.where(p["hflip"], FLAG_HFLIP, 0) | np.where(p["jitter"], FLAG_JITTER, 0) | np.where(p["gray"], FLAG_GRAY, 0)).astype(np.int32)
    rec["order"] = (ops << (4 * np.arange(4))).sum(axis=1).astype(np.int32)
    return torch.from_numpy(rec.view(np.int32).reshape(n, RECORD_INT32).copy())


def sample_view_params(sizes, generator: Optional[torch.Generator] = None, offsets=None) -> torch.Tensor:
    """Records of both views of every image, parameters drawn from `generator`: int32 [2B, 16]."""
    s = _sizes(sizes)
    return view_records(s, params_from_uniforms(s, draw_view_uniforms(len(s), generator)), offsets)


# ---- decode, pack, apply ------------------------------------------------------------------------------------------------------------
def pack_two_views(encoded, generator: Optional[torch.Generator] = None, lengths=None, threads: Optional[int] = None,
                   decode: str = "host") -> dict:
    """Decoded, packed batch with the records of its 2B views: {"data", "offsets", "xforms"} (see module doc).  Every image is decoded
    once and serves both of its views.  `encoded` / `lengths`: as `augment.decode_images` takes them.  decode="device": the form
    `augment.pack` documents, {"jpeg", "plans", "offsets", "host_pixels", "xforms"}, made without touching the GPU."""
    if _check_decode(decode):
        packed, sizes = _pack_device(_buffers(encoded, lengths, "decode_images"), threads)
        packed["xforms"] = sample_view_params(sizes, generator, packed["offsets"][:-1])
        return packed
    data, offsets, sizes = decode_images(encoded, lengths=lengths, threads=threads)
    return {"data": data, "offsets": offsets, "xforms": sample_view_params(sizes, generator, offsets[:-1])}


def collate_two_views(samples, generator: Optional[torch.Generator] = None, threads: Optional[int] = None, decode: str = "host") -> dict:
    """collate_fn for a dataset whose items are ENCODED images (bytes; the reference's `DatasetForSimCLRStyleTraining.load_image`
    input): returns the packed batch `SimCLR.train_step` takes."""
    return pack_two_views(list(samples), generator, threads=threads, decode=decode)


def is_packed(batch) -> bool:
    return isinstance(batch, dict) and ("data" in batch or is_device_packed(batch)) and "xforms" in batch


def apply(packed: dict, device=None) -> torch.Tensor:
    """fp32 [2B,3,224,224] on the device from a packed batch: rows 0 .. B-1 the first views, B .. 2B-1 the second (CPU tensors are
    copied first, asynchronously from pinned memory); enqueued on the current stream, no host synchronisation."""
    from . import ops

    if is_device_packed(packed):     # decode="device": a host synchronisation on the decode's status word (augment.decode_packed)
        data = decode_packed(packed, device)
        return ops.simclr_views(data, packed["xforms"].to(data.device, non_blocking=True))
    if device is None:
        device = packed["data"].device if packed["data"].is_cuda else torch.device("cuda", torch.cuda.current_device())
    return ops.simclr_views(packed["data"].to(device, non_blocking=True), packed["xforms"].to(device, non_blocking=True))
