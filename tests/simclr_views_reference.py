"""Torch-only restatement of the reference's SimCLR view pipeline (bioscanclip/util/dataset.py:314-325), the oracle of
clibd_amd.simclr_views / clibd_simclr_views_u8.  torchvision is not needed.

`float_view` is torchvision's tensor path for a float image (the float branch of transforms/_functional_tensor.py) in a chosen dtype,
nothing rounded between the stages: what the kernel implements.  `pil_view` is the path the reference actually runs — torchvision's PIL
backend, every stage rounding to uint8 — and is there to measure how far the two stand apart, never to gate the kernel.

A view is a plain dict: top, left, h, w, hflip, jitter, ops (the four operation ids 0 brightness, 1 contrast, 2 saturation, 3 hue in the
order they are applied), brightness, contrast, saturation, hue, gray, sigma."""
from __future__ import annotations

import itertools

import numpy as np
import torch
import torch.nn.functional as F

from tests import augment_reference as R

KSIZE = 21
ORDERS = list(itertools.permutations(range(4)))


def view_of(params: dict, r: int) -> dict:
    """row r of clibd_amd.simclr_views.params_from_uniforms's arrays as a view dict; the factors as the fp32 values a record stores"""
    v = {k: int(params[k][r]) for k in ("top", "left", "h", "w")}
    v.update({k: bool(params[k][r]) for k in ("hflip", "jitter", "gray")})
    v.update({k: float(np.float32(params[k][r])) for k in ("brightness", "contrast", "saturation", "hue", "sigma")})
    v["ops"] = tuple(int(o) for o in params["ops"][r])
    return v


def plain_view(top=0, left=0, h=224, w=224, **kw) -> dict:
    v = dict(top=top, left=left, h=h, w=w, hflip=False, jitter=False, gray=False, ops=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0,
             hue=0.0, sigma=0.1)
    v.update(kw)
    return v


def params_of(views, image=None) -> dict:
    """the arrays clibd_amd.simclr_views.view_records takes, from view dicts"""
    p = {k: np.array([v[k] for v in views]) for k in ("top", "left", "h", "w", "hflip", "jitter", "gray", "brightness", "contrast", "saturation", "hue", "sigma")}
    p["ops"] = np.array([v["ops"] for v in views], dtype=np.int64).reshape(len(views), 4)
    p["image"] = np.arange(len(views)) if image is None else np.asarray(image)
    return p


# ---- torchvision's tensor path, float branch ----------------------------------------------------------------------------------------
def gray_of(x: torch.Tensor) -> torch.Tensor:
    r, g, b = x.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def blend(a: torch.Tensor, b: torch.Tensor, f: float) -> torch.Tensor:
    return (f * a + (1.0 - f) * b).clamp(0, 1)


def brightness(x, f):
    return blend(x, torch.zeros_like(x), f)


def contrast(x, f):
    return blend(x, gray_of(x).mean(dim=(-3, -2, -1), keepdim=True), f)


def saturation(x, f):
    return blend(x, gray_of(x), f)


def rgb2hsv(x):
    r, g, b = x.unbind(dim=-3)
    maxc = x.max(dim=-3).values
    minc = x.min(dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def hsv2rgb(x):
    h, s, v = x.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * f)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    mask = i.unsqueeze(-3) == torch.arange(6).view(-1, 1, 1)
    a = torch.stack((torch.stack((v, q, p, p, t, v), dim=-3), torch.stack((t, v, v, q, p, p), dim=-3), torch.stack((p, p, t, v, v, q), dim=-3)), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(x.dtype), a)


def hue(x, f):
    hsv = rgb2hsv(x)
    h, s, v = hsv.unbind(dim=-3)
    return hsv2rgb(torch.stack(((h + f) % 1.0, s, v), dim=-3))


def gaussian_weights(sigma: float, dtype) -> torch.Tensor:
    k = torch.linspace(-(KSIZE // 2), KSIZE // 2, KSIZE, dtype=dtype)
    pdf = torch.exp(-0.5 * (k / sigma) ** 2)
    return pdf / pdf.sum()


def blur(x: torch.Tensor, sigma: float) -> torch.Tensor:
    """the separable 21-tap Gaussian on a reflect-padded [3, H, W] image, as explicit shifted sums: columns first, then rows"""
    w = gaussian_weights(sigma, x.dtype)
    half = KSIZE // 2
    H, W = x.shape[-2:]
    p = F.pad(x[None], (half, half, 0, 0), mode="reflect")[0]
    x = sum(w[k] * p[..., k:k + W] for k in range(KSIZE))
    p = F.pad(x[None], (0, 0, half, half), mode="reflect")[0]
    return sum(w[k] * p[..., k:k + H, :] for k in range(KSIZE))


def colour_ops(x: torch.Tensor, v: dict) -> torch.Tensor:
    fn = {0: (brightness, "brightness"), 1: (contrast, "contrast"), 2: (saturation, "saturation"), 3: (hue, "hue")}
    for op in v["ops"]:
        x = fn[op][0](x, v[fn[op][1]])
    return x


def crop_resample(img_u8: np.ndarray, v: dict, dtype) -> torch.Tensor:
    x = torch.from_numpy(np.array(img_u8, dtype=np.uint8)).permute(2, 0, 1).contiguous().to(dtype).div(255)
    x = R.resize(x[:, v["top"]:v["top"] + v["h"], v["left"]:v["left"] + v["w"]], 224, 224)
    return x.flip(-1) if v["hflip"] else x


def float_view(img_u8: np.ndarray, v: dict, dtype=torch.float32, blurred: bool = True) -> torch.Tensor:
    """[3, 224, 224] in `dtype`: crop, resample, flip -> colour jitter -> grayscale -> blur"""
    x = crop_resample(img_u8, v, dtype)
    if v["jitter"]:
        x = colour_ops(x, v)
    if v["gray"]:
        x = gray_of(x).expand(3, -1, -1).contiguous()
    return blur(x, v["sigma"]) if blurred else x


# ---- torchvision's PIL backend: what the reference's pipeline runs --------------------------------------------------------------------
def pil_hue(im, f: float):
    from PIL import Image

    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h = (np_h.astype(np.int64) + int(f * 255)) % 256       # the uint8 wrap-around of torchvision's `np_h += np.uint8(f * 255)`
    return Image.merge("HSV", (Image.fromarray(np_h.astype(np.uint8), "L"), s, v)).convert("RGB")


def pil_view(img_u8: np.ndarray, v: dict) -> torch.Tensor:
    """fp32 [3, 224, 224]: crop().resize(BILINEAR), ImageEnhance.{Brightness, Contrast, Color}, hue by the uint8 shift in HSV mode,
    convert("L"), the blur on the uint8 tensor with the result rounded, ToTensor."""
    from PIL import Image, ImageEnhance

    im = Image.fromarray(np.asarray(img_u8, dtype=np.uint8))
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
                im = pil_hue(im, v["hue"])
    if v["gray"]:
        g = np.array(im.convert("L"))
        im = Image.fromarray(np.dstack([g, g, g]), "RGB")
    x = torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().to(torch.float32)
    x = blur(x, v["sigma"]).round().clamp(0, 255).to(torch.uint8)
    return x.to(torch.float32).div(255)


# ---- the seeded fixture of the float-against-PIL comparison --------------------------------------------------------------------------
def fixture_image(h: int = 256, w: int = 341, seed: int = 0) -> np.ndarray:
    """smooth colour gradients plus noise, so that resampling, hue and blur errors would all show"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (127 + 100 * np.sin(yy[..., None] * 0.05 + xx[..., None] * 0.03 + 2.1 * np.arange(3))).astype(np.int64)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def gap_views(H: int = 256, W: int = 341, seed: int = 7) -> list:
    """one seeded parameter set per order of the four operations (24): sampler boxes, flips, factors, sigma; jitter on, grayscale off"""
    from clibd_amd import simclr_views as V

    p = V.params_from_uniforms([(H, W)] * 12, V.draw_view_uniforms(12, torch.Generator().manual_seed(seed)))
    out = []
    for r, order in enumerate(ORDERS):
        v = view_of(p, r)
        v.update(jitter=True, gray=False, ops=order)
        out.append(v)
    return out


def views_of_records(xforms) -> list:
    """the view dicts of int32 [n, 16] records (struct clibd_view_xform), e.g. what pack_two_views drew"""
    from clibd_amd import simclr_views as V

    out = []
    for r in xforms.cpu().numpy().view(V._RECORD).reshape(-1):
        v = {k: int(r[k]) for k in ("top", "left", "h", "w")}
        v.update(hflip=bool(r["flags"] & V.FLAG_HFLIP), jitter=bool(r["flags"] & V.FLAG_JITTER), gray=bool(r["flags"] & V.FLAG_GRAY),
                 ops=tuple((int(r["order"]) >> (4 * j)) & 15 for j in range(4)))
        v.update({k: float(r[k]) for k in ("brightness", "contrast", "saturation", "hue", "sigma")})
        out.append(v)
    return out
