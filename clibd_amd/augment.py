"""The dataset's image transforms on the device (f1 batch contract, images): the host decodes JPEG / PNG bytes and packs the uint8
pixels; the transform chain of the reference's dataset runs as HIP (clibd_image_transform_u8, csrc/augment.hip).

    training (util/dataset.py:185-195): ToTensor -> Resize(256, antialias) -> RandomResizedCrop(224, antialias) -> RandomHorizontalFlip
                                        -> RandomVerticalFlip -> RandomRotation((-45, 45))
    eval     (util/dataset.py:216-224): ToTensor -> Resize(256, antialias) -> CenterCrop(224)

The random parameters follow torchvision's samplers in distribution (not stream for stream: the reference's stream depends on its
DataLoader workers): `draw_uniforms` draws them in bulk from a seeded torch.Generator, `params_from_uniforms` turns them into crop
boxes, flips and angles.  A packed batch is a dict of tensors {"data", "offsets", "xforms"}, so `data.DevicePrefetcher` moves it as it
is; `apply` turns it into fp32 [B,3,224,224] on the device without a host synchronisation.

With decode="device" (opt-in) the baseline JPEG streams of a batch stay compressed on the host: the batch is {"jpeg", "plans", "offsets",
"host_pixels", "xforms"}, and `apply` decodes them with HIP kernels (clibd_jpeg_decode_u8, csrc/jpeg.hip) into the same packed
pixels, equal to PIL's byte for byte, with a host synchronisation on the decode's status word (`decode_packed`).
"""
from __future__ import annotations

import concurrent.futures as cf
import io
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

OUT = 224
RESIZE = 256
CROP_MAX = 384                   # crop box side the kernel accepts (RandomResizedCrop of a 256-short-side image: <= 342)
DOWN_MAX = 16                    # resize factor per axis the kernel accepts (a short side up to 4096)
MAX_THREADS = 16
FLAG_HFLIP, FLAG_VFLIP, FLAG_ROTATE = 1, 2, 4
SCALE, RATIO, DEGREES = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), (-45.0, 45.0)
ATTEMPTS = 10
N_UNIFORMS = 2 * ATTEMPTS + 2 + 3   # per attempt (area, log-ratio); crop top, left; hflip, vflip, angle
RECORD_INT32 = 18                   # struct clibd_image_xform (include/clibd_hip.h): 72 bytes

_RECORD = np.dtype([("offset", "<i8"), ("H0", "<i4"), ("W0", "<i4"), ("H1", "<i4"), ("W1", "<i4"), ("top", "<i4"), ("left", "<i4"),
                    ("h", "<i4"), ("w", "<i4"), ("flags", "<i4"), ("reserved", "<i4"), ("theta", "<f4", (6,))])
assert _RECORD.itemsize == 4 * RECORD_INT32


# ---- sizes --------------------------------------------------------------------------------------------------------------------------
def resize_size(H0: int, W0: int, size: int = RESIZE) -> tuple:
    """torchvision Resize(size) with an int size: the short side becomes `size`, the long one int(size * long / short)."""
    short, long = (W0, H0) if W0 <= H0 else (H0, W0)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if W0 <= H0 else (new_short, new_long)


def center_crop_offsets(H1: int, W1: int, size: int = OUT) -> tuple:
    """torchvision CenterCrop: top = int(round((H1 - size) / 2)) (half to even), left likewise."""
    return int(round((H1 - size) / 2.0)), int(round((W1 - size) / 2.0))


def _sizes(sizes) -> np.ndarray:
    s = np.asarray(sizes.cpu() if torch.is_tensor(sizes) else sizes, dtype=np.int64).reshape(-1, 2)
    if len(s) == 0:
        raise ValueError("augment: empty batch")
    if (s < 1).any():
        raise ValueError("augment: image sizes must be positive")
    return s


# ---- random parameters --------------------------------------------------------------------------------------------------------------
def draw_uniforms(B: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """float64 [B, N_UNIFORMS] uniforms in [0, 1): everything the training transform of B images draws."""
    return torch.rand((B, N_UNIFORMS), dtype=torch.float64, generator=generator)


def _randint(u: float, n: int) -> int:
    """torch.randint(0, n) from one uniform: min(floor(u n), n - 1)."""
    return min(int(math.floor(u * n)), n - 1)


def crop_box(H1: int, W1: int, u: Sequence[float]) -> tuple:
    """torchvision RandomResizedCrop.get_params(scale=(0.08, 1), ratio=(3/4, 4/3)) on an H1 x W1 image with uniforms
    u[0:2*ATTEMPTS] (area, log-ratio per attempt) and u[2*ATTEMPTS : 2*ATTEMPTS+2] (top, left): (top, left, h, w)."""
    area = H1 * W1
    lr0, lr1 = math.log(RATIO[0]), math.log(RATIO[1])
    for a in range(ATTEMPTS):
        target_area = area * (SCALE[0] + (SCALE[1] - SCALE[0]) * u[2 * a])
        aspect_ratio = math.exp(lr0 + (lr1 - lr0) * u[2 * a + 1])
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W1 and 0 < h <= H1:
            return _randint(u[2 * ATTEMPTS], H1 - h + 1), _randint(u[2 * ATTEMPTS + 1], W1 - w + 1), h, w
    in_ratio = float(W1) / float(H1)         # fallback: central crop, ratio clamped
    if in_ratio < min(RATIO):
        w = W1
        h = int(round(w / min(RATIO)))
    elif in_ratio > max(RATIO):
        h = H1
        w = int(round(h * max(RATIO)))
    else:
        w, h = W1, H1
    return (H1 - h) // 2, (W1 - w) // 2, h, w


def rotation_theta(angle: float) -> np.ndarray:
    """fp32 [cos a, -sin a, 0, sin a, cos a, 0], a = radians(angle): torchvision's _get_inverse_affine_matrix at -angle (float64, then fp32)."""
    a = math.radians(angle)
    return np.array([math.cos(a), -math.sin(a), 0.0, math.sin(a), math.cos(a), 0.0], dtype=np.float64).astype(np.float32)


def params_from_uniforms(sizes, uniforms) -> dict:
    """Training parameters of every image from its uniforms (pure): Resize size, crop box (in the resized image), flips, angle."""
    s = _sizes(sizes)
    u = np.asarray(uniforms.cpu() if torch.is_tensor(uniforms) else uniforms, dtype=np.float64).reshape(len(s), N_UNIFORMS)
    B = len(s)
    H1, W1, top, left, h, w = (np.empty(B, dtype=np.int64) for _ in range(6))
    for i in range(B):
        H1[i], W1[i] = resize_size(int(s[i, 0]), int(s[i, 1]))
        top[i], left[i], h[i], w[i] = crop_box(int(H1[i]), int(W1[i]), u[i].tolist())
    k = 2 * ATTEMPTS + 2
    return {"H1": H1, "W1": W1, "top": top, "left": left, "h": h, "w": w, "hflip": u[:, k] < 0.5, "vflip": u[:, k + 1] < 0.5,
            "angle": DEGREES[0] + (DEGREES[1] - DEGREES[0]) * u[:, k + 2]}


# ---- records ------------------------------------------------------------------------------------------------------------------------
def _packed_offsets(s: np.ndarray) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(s[:, 0] * s[:, 1] * 3)]).astype(np.int64)


def _records(s: np.ndarray, p: dict, offsets, rotate: bool) -> torch.Tensor:
    B = len(s)
    offs = _packed_offsets(s)[:B] if offsets is None else np.asarray(offsets, dtype=np.int64).reshape(-1)[:B]
    if len(offs) != B or (offs < 0).any():
        raise ValueError("augment: one non-negative byte offset per image")
    for name in ("h", "w"):
        if (p[name] < 1).any() or (p[name] > CROP_MAX).any():
            raise ValueError(f"augment: crop {name} outside [1, {CROP_MAX}]")
    if (p["top"] < 0).any() or (p["left"] < 0).any() or (p["top"] + p["h"] > p["H1"]).any() or (p["left"] + p["w"] > p["W1"]).any():
        raise ValueError("augment: crop box outside the resized image")
    if (s[:, 0] > DOWN_MAX * p["H1"]).any() or (s[:, 1] > DOWN_MAX * p["W1"]).any() or (s > 65535).any():
        raise ValueError(f"augment: images larger than {DOWN_MAX * RESIZE} pixels on the short side are not supported")
    rec = np.zeros(B, dtype=_RECORD)
    rec["offset"], rec["H0"], rec["W0"], rec["H1"], rec["W1"] = offs, s[:, 0], s[:, 1], p["H1"], p["W1"]
    rec["top"], rec["left"], rec["h"], rec["w"] = p["top"], p["left"], p["h"], p["w"]
    flags = np.zeros(B, dtype=np.int32)
    if "hflip" in p:
        flags |= np.where(p["hflip"], FLAG_HFLIP, 0).astype(np.int32)
        flags |= np.where(p["vflip"], FLAG_VFLIP, 0).astype(np.int32)
    if rotate:
        flags |= FLAG_ROTATE
        rec["theta"] = np.stack([rotation_theta(float(a)) for a in p["angle"]])
    rec["flags"] = flags
    return torch.from_numpy(rec.view(np.int32).reshape(B, RECORD_INT32).copy())


def train_records(sizes, params: dict, offsets=None, rotate: bool = True) -> torch.Tensor:
    """int32 [B, 18] records of the training transform from `params_from_uniforms`'s parameters (rotate=False: no rotation stage)."""
    return _records(_sizes(sizes), params, offsets, rotate)


def sample_train_params(sizes, generator: Optional[torch.Generator] = None, offsets=None) -> torch.Tensor:
    """Records of the training transform: Resize(256) -> RandomResizedCrop(224) -> flips -> RandomRotation((-45, 45)), parameters drawn
    from `generator`.  offsets: byte offset of each image in the packed buffer (default: packed back to back, as `decode_images` does)."""
    s = _sizes(sizes)
    return train_records(s, params_from_uniforms(s, draw_uniforms(len(s), generator)), offsets)


def eval_params(sizes, offsets=None) -> torch.Tensor:
    """Records of the eval transform: Resize(256) -> CenterCrop(224)."""
    s = _sizes(sizes)
    B = len(s)
    p = {k: np.empty(B, dtype=np.int64) for k in ("H1", "W1", "top", "left")}
    for i in range(B):
        p["H1"][i], p["W1"][i] = resize_size(int(s[i, 0]), int(s[i, 1]))
        p["top"][i], p["left"][i] = center_crop_offsets(int(p["H1"][i]), int(p["W1"][i]))
    p["h"] = np.full(B, OUT, dtype=np.int64)
    p["w"] = np.full(B, OUT, dtype=np.int64)
    return _records(s, p, offsets, rotate=False)


# ---- decode and pack ----------------------------------------------------------------------------------------------------------------
def default_threads() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:   # pragma: no cover
        n = os.cpu_count() or 1
    return max(1, min(MAX_THREADS, n))


def _decode_one(buf) -> np.ndarray:
    from PIL import Image

    if len(buf) == 0:
        raise ValueError("decode_images: empty image")
    with Image.open(io.BytesIO(bytes(buf))) as im:
        if im.mode != "RGB":
            raise ValueError(f"decode_images: {im.mode} image (the model takes RGB)")
        a = np.asarray(im)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("decode_images: empty image")
    return a


def decode_images(encoded, lengths=None, threads: Optional[int] = None, pin: Optional[bool] = None):
    """Decode JPEG / PNG bytes with PIL on up to 16 threads and pack the RGB HWC uint8 pixels back to back.

    encoded: a list of `bytes`, or the reference's HDF5 layout (`image` uint8 [B, Lmax] zero-padded, `lengths` = its `image_mask`).
    Returns (data uint8 [N] (pinned when a GPU is present), offsets int64 [B+1], sizes int64 [B, 2] = (H, W))."""
    bufs = _buffers(encoded, lengths, "decode_images")
    nthreads = max(1, min(MAX_THREADS, threads or default_threads()))
    with cf.ThreadPoolExecutor(max_workers=nthreads) as ex:
        arrays = list(ex.map(_decode_one, bufs))
        sizes = np.array([a.shape[:2] for a in arrays], dtype=np.int64)
        offsets = _packed_offsets(sizes)
        if pin is None:
            pin = torch.cuda.is_available()
        data = torch.empty((int(offsets[-1]),), dtype=torch.uint8, pin_memory=bool(pin))
        flat = data.numpy()

        def put(i):
            flat[offsets[i]:offsets[i + 1]] = arrays[i].reshape(-1)

        list(ex.map(put, range(len(arrays))))
    return data, torch.from_numpy(offsets), torch.from_numpy(sizes)


# ---- decode on the device -------------------------------------------------------------------------------------------------------------
# Baseline JPEG streams are planned on the host (clibd_jpeg_plan: markers, tables, H and W; no GPU) and decoded by HIP kernels
# (clibd_jpeg_decode_u8, csrc/jpeg.hip) into the same packed buffer; every other stream takes `_decode_one`.  DESIGN §3.15.
PLAN_BYTES = 4096                # struct clibd_jpeg_record (include/clibd_hip_jpeg.h)
_PLAN_HEAD = np.dtype([("reason", "<i4"), ("H", "<i4"), ("W", "<i4"), ("sampling", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("blocks", "<i4"),
                       ("restart_interval", "<i4"), ("scan_begin", "<i4"), ("stream_len", "<i4"), ("stream_begin", "<i8"), ("coef_begin", "<i8")])
_PLAN = np.dtype(_PLAN_HEAD.descr + [("tables", "u1", (PLAN_BYTES - _PLAN_HEAD.itemsize,))])
assert _PLAN_HEAD.itemsize == 56 and _PLAN.itemsize == PLAN_BYTES
DECODERS = ("host", "device")


def _check_decode(decode: str) -> bool:
    if decode not in DECODERS:
        raise ValueError(f"augment: decode must be one of {DECODERS}, not {decode!r}")
    return decode == "device"


def _buffers(encoded, lengths, who: str) -> list:
    if lengths is not None:
        enc = np.asarray(encoded.cpu() if torch.is_tensor(encoded) else encoded, dtype=np.uint8)
        lens = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
        if enc.ndim != 2 or len(enc) != len(lens) or (lens < 0).any() or (lens > enc.shape[1]).any():
            raise ValueError(f"{who}: image [B, Lmax] with one length in [0, Lmax] per row expected")
        bufs = [enc[i, :lens[i]] for i in range(len(lens))]
    else:
        bufs = list(encoded)
    if not bufs:
        raise ValueError(f"{who}: empty batch")
    return bufs


def plan_streams(bufs, threads: Optional[int] = None) -> np.ndarray:
    """One struct clibd_jpeg_record per stream (a numpy record array [B] of PLAN_BYTES each), placement fields zero.  Host only."""
    import ctypes

    from . import _lib

    lib = _lib.load()
    plans = np.zeros(len(bufs), dtype=_PLAN)
    base = plans.ctypes.data

    def one(i):
        b = bufs[i]
        a = np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
        if lib.clibd_jpeg_plan(ctypes.c_void_p(a.ctypes.data if a.size else None), a.size, ctypes.c_void_p(base + i * PLAN_BYTES)) < 0:
            raise RuntimeError("clibd_jpeg_plan failed")   # a null record: cannot happen here

    nthreads = max(1, min(MAX_THREADS, threads or default_threads()))
    with cf.ThreadPoolExecutor(max_workers=nthreads) as ex:
        list(ex.map(one, range(len(bufs))))
    return plans


def _pack_device(bufs, threads: Optional[int] = None, pin: Optional[bool] = None):
    """The device-decode form of a batch, made without touching the GPU: ({"jpeg", "plans", "offsets", "host_pixels"}, sizes).
    Streams the plan does not call eligible are decoded here with `_decode_one` (its exceptions included)."""
    plans = plan_streams(bufs, threads)
    B = len(bufs)
    device_idx = np.nonzero(plans["reason"] == 0)[0]
    host_idx = np.nonzero(plans["reason"] != 0)[0]
    nthreads = max(1, min(MAX_THREADS, threads or default_threads()))
    with cf.ThreadPoolExecutor(max_workers=nthreads) as ex:
        arrays = list(ex.map(lambda i: _decode_one(bufs[i]), host_idx))
    sizes = np.stack([plans["H"], plans["W"]], axis=1).astype(np.int64)
    for i, a in zip(host_idx, arrays):
        sizes[i] = a.shape[:2]
    offsets = _packed_offsets(sizes)
    if pin is None:
        pin = torch.cuda.is_available()
    lens = np.array([len(bufs[i]) for i in device_idx], dtype=np.int64)
    begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    jpeg = torch.empty((int(begin[-1]),), dtype=torch.uint8, pin_memory=bool(pin and begin[-1] > 0))
    flat = jpeg.numpy()
    for k, i in enumerate(device_idx):
        flat[begin[k]:begin[k + 1]] = np.frombuffer(bufs[i], dtype=np.uint8) if isinstance(bufs[i], (bytes, bytearray, memoryview)) else bufs[i]
    plans["stream_begin"][device_idx] = begin[:-1]
    blocks = np.where(plans["reason"] == 0, plans["blocks"], 0).astype(np.int64)
    plans["coef_begin"] = np.concatenate([[0], np.cumsum(blocks)])[:B]
    nhost = int(sum(a.size for a in arrays))
    host_pixels = torch.empty((nhost,), dtype=torch.uint8, pin_memory=bool(pin and nhost > 0))
    if arrays:
        host_pixels.numpy()[:] = np.concatenate([a.reshape(-1) for a in arrays])
    packed = {"jpeg": jpeg, "plans": torch.from_numpy(plans.view(np.uint8).reshape(B, PLAN_BYTES)), "offsets": torch.from_numpy(offsets),
              "host_pixels": host_pixels}
    return packed, torch.from_numpy(sizes)


def is_device_packed(image) -> bool:
    return isinstance(image, dict) and "jpeg" in image and "plans" in image and "offsets" in image


def decode_packed(packed: dict, device=None, return_status: bool = False):
    """The pixels of a device-decode batch: uint8 [N] on the device, the layout `decode_images` returns.  Copies the compressed bytes,
    launches the decode, copies the host-decoded slices in, reads the status word once and decodes again with `_decode_one` every image
    the device gave up on (a damaged file then behaves as on the host path, PIL's exception included).  return_status: also the int32 [B]
    status as the device left it (0: decoded there; a plan's reason: decoded on the host from the start; >= 32: stopped on the device and
    decoded again on the host).  Host synchronisations: the status read after the launch; and, when the batch's tensors were moved to the
    device beforehand (a prefetcher), two small reads before it, of the records' 56-byte heads and of the offsets."""
    from . import ops

    if device is None:
        device = packed["jpeg"].device if packed["jpeg"].is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    plans = packed["plans"]
    B = plans.shape[0]
    head = plans[:, :_PLAN_HEAD.itemsize].cpu().contiguous().numpy().view(_PLAN_HEAD).reshape(B)
    offsets = packed["offsets"].cpu().numpy()
    on_device = head["reason"] == 0
    out = torch.empty((int(offsets[-1]),), dtype=torch.uint8, device=device)
    status = None
    jpeg = packed["jpeg"].to(device, non_blocking=True)
    if on_device.any():
        total_blocks = int(head["blocks"][on_device].astype(np.int64).sum())
        status = ops.jpeg_decode(jpeg, plans.to(device, non_blocking=True), packed["offsets"].to(device, non_blocking=True), out, total_blocks)
    host_pixels = packed["host_pixels"].to(device, non_blocking=True)
    at = 0
    for i in np.nonzero(~on_device)[0]:
        n = int(offsets[i + 1] - offsets[i])
        out[int(offsets[i]):int(offsets[i + 1])].copy_(host_pixels[at:at + n])
        at += n
    st = np.where(on_device, 0, head["reason"]).astype(np.int32)
    if status is not None:
        st = status.cpu().numpy()                                   # the synchronisation after the launch
        for i in np.nonzero(on_device & (st != 0))[0]:
            b0 = int(head["stream_begin"][i])
            a = _decode_one(packed["jpeg"][b0:b0 + int(head["stream_len"][i])].cpu().numpy())
            if a.shape[:2] != (int(head["H"][i]), int(head["W"][i])):
                raise ValueError("decode_images: the image's size differs from its frame header")
            out[int(offsets[i]):int(offsets[i + 1])].copy_(torch.from_numpy(a.reshape(-1).copy()))
    return (out, torch.from_numpy(st)) if return_status else out


def decode_images_device(encoded, lengths=None, device=None, threads: Optional[int] = None, return_status: bool = False):
    """`decode_images` with the baseline JPEG streams decoded on the device: (data uint8 [N] on the device, offsets int64 [B+1],
    sizes int64 [B, 2]), equal to `decode_images`'s byte for byte.  Takes both of its input layouts.  return_status: a fourth entry,
    `decode_packed`'s status (which images the device decoded itself)."""
    packed, sizes = _pack_device(_buffers(encoded, lengths, "decode_images"), threads)
    if return_status:
        data, status = decode_packed(packed, device, return_status=True)
        return data, packed["offsets"], sizes, status
    return decode_packed(packed, device), packed["offsets"], sizes


def pack(encoded, train: bool, generator: Optional[torch.Generator] = None, lengths=None, threads: Optional[int] = None,
         decode: str = "host") -> dict:
    """Decoded, packed batch with its records: {"data", "offsets", "xforms"} (see module doc).  decode="device": the batch with its
    baseline JPEG streams still compressed, {"jpeg", "plans", "offsets", "host_pixels", "xforms"}, made without touching the GPU;
    `apply` decodes it there."""
    if _check_decode(decode):
        packed, sizes = _pack_device(_buffers(encoded, lengths, "decode_images"), threads)
        offsets = packed["offsets"]
        packed["xforms"] = sample_train_params(sizes, generator, offsets[:-1]) if train else eval_params(sizes, offsets[:-1])
        return packed
    data, offsets, sizes = decode_images(encoded, lengths=lengths, threads=threads)
    xforms = sample_train_params(sizes, generator, offsets[:-1]) if train else eval_params(sizes, offsets[:-1])
    return {"data": data, "offsets": offsets, "xforms": xforms}


def _stack(items):
    if torch.is_tensor(items[0]):
        return torch.stack(list(items))
    if isinstance(items[0], (int, np.integer)):
        return torch.tensor(np.asarray(items, dtype=np.int64))
    if isinstance(items[0], np.ndarray):
        return torch.from_numpy(np.stack(items))
    if isinstance(items[0], dict):
        return {k: [d[k] for d in items] for k in items[0]}
    return list(items)


def collate_encoded(samples, train: bool, generator: Optional[torch.Generator] = None, threads: Optional[int] = None, decode: str = "host"):
    """collate_fn for the reference's 7-tuples whose image entry is the ENCODED image (bytes): returns the reference's batch
    (processid, image, dna, input_ids, token_type_ids, attention_mask, label) with image = {"data", "offsets", "xforms"}, or with
    decode="device" the form `pack` documents (no GPU is touched here: the function runs in loader workers).
    Labels are stacked into a tensor (training) or gathered into {level: [labels]} (eval label dicts), as default_collate does."""
    cols = list(zip(*samples))
    if len(cols) != 7:
        raise ValueError("collate_encoded: samples must be the reference's 7-tuples")
    image = pack(list(cols[1]), train, generator, threads=threads, decode=decode)
    return (list(cols[0]), image, _stack(cols[2]), _stack(cols[3]), _stack(cols[4]), _stack(cols[5]), _stack(cols[6]))


def is_packed(image) -> bool:
    return isinstance(image, dict) and ("data" in image or is_device_packed(image)) and "xforms" in image


def apply(packed: dict, device=None) -> torch.Tensor:
    """fp32 [B,3,224,224] on the device from a packed batch (CPU tensors are copied first, asynchronously from pinned memory);
    enqueued on the current stream, no host synchronisation."""
    from . import ops

    if is_device_packed(packed):     # decode="device": a host synchronisation on the decode's status word (see decode_packed)
        data = decode_packed(packed, device)
        return ops.image_transform(data, packed["xforms"].to(data.device, non_blocking=True))
    if device is None:
        device = packed["data"].device if packed["data"].is_cuda else torch.device("cuda", torch.cuda.current_device())
    return ops.image_transform(packed["data"].to(device, non_blocking=True), packed["xforms"].to(device, non_blocking=True))
