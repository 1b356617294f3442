"""Torch-only restatement of the reference dataset's image transforms (bioscanclip/util/dataset.py:185-195 training, :216-224 eval),
the oracle of clibd_amd.augment / clibd_image_transform_u8.  torchvision is not needed: every step is written with the torch ops
torchvision calls (F.interpolate antialiased bilinear, tensor slicing, flip, grid_sample nearest)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from clibd_amd.augment import ATTEMPTS, RATIO, SCALE, center_crop_offsets, resize_size, rotation_theta


def to_tensor(img_u8: np.ndarray) -> torch.Tensor:
    """ToTensor: HWC uint8 -> CHW fp32 u8 / 255."""
    return torch.from_numpy(np.array(img_u8, dtype=np.uint8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def resize(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Resize to (H, W) with antialias; a size that does not change returns the image (torchvision's early return)."""
    if tuple(x.shape[-2:]) == (H, W):
        return x
    return F.interpolate(x[None], size=(H, W), mode="bilinear", align_corners=False, antialias=True)[0]


def affine_grid(theta: np.ndarray, H: int = 224, W: int = 224) -> torch.Tensor:
    """torchvision _gen_affine_grid: base grid x = -W/2+0.5 .. W/2-0.5 (y likewise) times theta^T / [W/2, H/2]."""
    t = torch.from_numpy(np.asarray(theta, dtype=np.float32)).view(1, 2, 3)
    base = torch.empty(1, H, W, 3)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + 0.5, W * 0.5 - 0.5, steps=W))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + 0.5, H * 0.5 - 0.5, steps=H).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = t.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H])
    return base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)


def rotate(x: torch.Tensor, angle: float) -> torch.Tensor:
    """F.rotate(img, angle, NEAREST, expand=False, center=None, fill=0)."""
    grid = affine_grid(rotation_theta(angle), x.shape[-2], x.shape[-1])
    return F.grid_sample(x[None], grid, mode="nearest", padding_mode="zeros", align_corners=False)[0]


def rotation_source(angle: float, H: int = 224, W: int = 224) -> torch.Tensor:
    """[H, W, 2] unrounded source coordinates (x, y) of every output pixel: ((g + 1) * size - 1) / 2."""
    g = affine_grid(rotation_theta(angle), H, W)[0]
    return torch.stack([((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2], dim=-1)


def train_chain(img_u8, top, left, h, w, hflip=False, vflip=False, angle=None) -> torch.Tensor:
    """ToTensor -> Resize(256) -> crop (top, left, h, w) resampled to 224 x 224 -> flips -> rotation (angle None: none)."""
    x = to_tensor(img_u8)
    x = resize(x, *resize_size(*x.shape[-2:]))
    x = resize(x[:, top:top + h, left:left + w], 224, 224)
    if hflip:
        x = x.flip(-1)
    if vflip:
        x = x.flip(-2)
    if angle is not None:
        x = rotate(x, angle)
    return x


def eval_chain(img_u8) -> torch.Tensor:
    """ToTensor -> Resize(256) -> CenterCrop(224)."""
    x = to_tensor(img_u8)
    x = resize(x, *resize_size(*x.shape[-2:]))
    top, left = center_crop_offsets(*x.shape[-2:])
    return x[:, top:top + 224, left:left + 224].contiguous()


def get_params(height: int, width: int, uniforms) -> tuple:
    """torchvision RandomResizedCrop.get_params(img, scale=(0.08, 1.0), ratio=(3/4, 4/3)) restated with its draws taken from `uniforms`
    in order (area, log-ratio for each attempt, then top, left): torch.empty(1).uniform_(a, b) = a + (b - a) u, randint(0, n) = min(floor(u n), n - 1)."""
    it = iter(uniforms)
    area = height * width
    log_ratio = (math.log(RATIO[0]), math.log(RATIO[1]))
    for _ in range(10):
        target_area = area * (SCALE[0] + (SCALE[1] - SCALE[0]) * next(it))
        aspect_ratio = math.exp(log_ratio[0] + (log_ratio[1] - log_ratio[0]) * next(it))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            rest = list(uniforms)[2 * ATTEMPTS:]
            i = min(math.floor(rest[0] * (height - h + 1)), height - h)
            j = min(math.floor(rest[1] * (width - w + 1)), width - w)
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(RATIO):
        w = width
        h = int(round(w / min(RATIO)))
    elif in_ratio > max(RATIO):
        h = height
        w = int(round(h * max(RATIO)))
    else:
        w = width
        h = height
    i = (height - h) // 2
    j = (width - w) // 2
    return i, j, h, w
