"""CPU checks of the SimCLR view generator: the third header (include/clibd_hip_views.h) and its binding table, host-side validation of
the C entry, the new unit's scratch-free kernels, the sampler of clibd_amd.simclr_views, and the oracle itself
(tests/simclr_views_reference.py) pinned against sources that share no code with the kernel: colorsys, PIL.ImageEnhance, F.conv2d, and
the PIL path the reference runs."""
import colorsys
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clibd_amd import simclr_views as V
from tests import simclr_views_reference as S

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "clibd_hip_views.h"


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_views_header_symbols_record_layout_and_build_unit():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == ["clibd_simclr_views_u8", "clibd_simclr_views_workspace_bytes"]
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    # the record is 64 bytes, as the numpy mirror lays it out
    assert V._RECORD.itemsize == 64 and V._RECORD.fields["brightness"][1] == 40 and V._RECORD.fields["sigma"][1] == 56
    assert "} clibd_view_xform;" in HEADER.read_text() and "/* 64 bytes */" in HEADER.read_text()
    assert HEADER in build._deps() and "views" in build.SOURCES


def test_views_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    need = L.clibd_simclr_views_workspace_bytes(4)
    assert need >= 4 * 3 * 224 * 224 * 4 and need % 16 == 0
    assert L.clibd_simclr_views_workspace_bytes(0) == 0 and L.clibd_simclr_views_workspace_bytes(-3) == 0
    assert L.clibd_simclr_views_workspace_bytes(8) > need

    def call(data=P(4096), xf=P(8192), n=4, out=P(16384), ws=P(32768), nbytes=need):
        return L.clibd_simclr_views_u8(data, 1 << 20, xf, n, out, ws, nbytes, None)

    for kw, word in ((dict(data=None), b"null"), (dict(xf=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
                     (dict(n=0), b"n must"), (dict(n=-2), b"n must"), (dict(xf=P(8192 + 4)), b"alignment"), (dict(out=P(16384 + 8)), b"alignment"),
                     (dict(ws=P(32768 + 8)), b"alignment"), (dict(nbytes=need - 1), b"workspace too small"), (dict(nbytes=0), b"workspace too small")):
        assert call(**kw) == -1, kw
        assert word in L.clibd_last_error(), (kw, L.clibd_last_error())


def test_views_unit_uses_no_scratch():
    """Every kernel of csrc/views.hip keeps its working set in registers (the parse of tests/test_abi.py::test_hot_kernels_use_no_scratch)."""
    from clibd_amd import build

    rows = [(k["name"], k["scratch"]) for k in build.resource_usage("views")]
    names = " ".join(n for n, _ in rows)
    for k in ("views_weights_kernel", "views_resample_kernel", "views_finish_kernel"):
        assert k in names, (k, names)
    assert not [(n, s) for n, s in rows if s > 0], rows


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
SIZES = [(256, 341), (224, 224), (37, 53), (600, 800)]


def test_sampler_ranges_repeat_and_views_differ():
    sizes = SIZES * 16
    B = len(sizes)
    u = V.draw_view_uniforms(B, torch.Generator().manual_seed(3))
    assert u.dtype == torch.float64 and tuple(u.shape) == (B, 2, V.N_UNIFORMS) and V.N_UNIFORMS == 33
    assert torch.equal(u, V.draw_view_uniforms(B, torch.Generator().manual_seed(3)))
    p = V.params_from_uniforms(sizes, u)
    q = V.params_from_uniforms(sizes, u.clone())
    assert all(np.array_equal(p[k], q[k]) for k in p)          # pure
    assert all(len(p[k]) == 2 * B for k in p)
    assert np.array_equal(p["image"], np.concatenate([np.arange(B), np.arange(B)]))
    for k in ("brightness", "contrast", "saturation"):
        assert (p[k] >= 0.2).all() and (p[k] <= 1.8).all() and p[k].std() > 0.3
    assert (np.abs(p["hue"]) <= 0.2).all() and (p["sigma"] >= 0.1).all() and (p["sigma"] < 2.0).all()
    assert (np.sort(p["ops"], axis=1) == np.arange(4)).all()
    H0, W0 = np.array(sizes)[p["image"]].T
    assert (p["top"] >= 0).all() and (p["left"] >= 0).all() and (p["top"] + p["h"] <= H0).all() and (p["left"] + p["w"] <= W0).all()
    rec = V.view_records(sizes, p)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (2 * B, 16)
    assert torch.equal(rec, V.sample_view_params(sizes, torch.Generator().manual_seed(3)))
    # both views of a sample read the same pixels, with parameters of their own
    r = rec.numpy().view(V._RECORD).reshape(-1)
    assert np.array_equal(r["offset"][:B], r["offset"][B:]) and np.array_equal(r["H0"][:B], r["H0"][B:])
    assert all(not torch.equal(rec[i], rec[B + i]) for i in range(B))
    assert (r["order"] == [V.pack_order(o) for o in p["ops"]]).all() and (r["reserved"] == 0).all()


def test_sampler_thresholds():
    def one(**at):
        u = np.full((1, 2, V.N_UNIFORMS), 0.5)
        for k, v in at.items():
            u[0, 0, getattr(V, k)] = v
        return {k: v[0] for k, v in V.params_from_uniforms([(256, 341)], u).items()}

    assert one(U_HFLIP=0.4999)["hflip"] and not one(U_HFLIP=0.5)["hflip"]
    assert one(U_JITTER=0.8)["jitter"] and not one(U_JITTER=0.8000001)["jitter"] and one(U_JITTER=0.0)["jitter"]   # skipped when u > 0.8
    assert one(U_GRAY=0.1999)["gray"] and not one(U_GRAY=0.2)["gray"]
    assert one(U_SIGMA=0.0)["sigma"] == 0.1 and abs(one(U_SIGMA=0.5)["sigma"] - 1.05) < 1e-12
    lo, hi = one(U_FACTORS=0.0), one(U_FACTORS=1.0 - 2.0 ** -53)
    assert lo["brightness"] == 0.2 and abs(hi["brightness"] - 1.8) < 1e-12
    u = np.full((1, 2, V.N_UNIFORMS), 0.0)
    assert V.params_from_uniforms([(256, 341)], u)["hue"][0] == -0.2
    # the crop box is augment.crop_box on the ORIGINAL image (no Resize(256) in this pipeline)
    from clibd_amd.augment import crop_box

    uu = V.draw_view_uniforms(1, torch.Generator().manual_seed(11)).numpy()
    p = V.params_from_uniforms([(600, 800)], uu)
    assert (p["top"][1], p["left"][1], p["h"][1], p["w"][1]) == crop_box(600, 800, uu[0, 1, :22].tolist())


def test_sampler_reaches_all_orders_equally_often():
    grid = [(k + 0.5) / 12 for k in range(12)]
    counts = {}
    for a in grid:
        for b in grid:
            for c in grid:
                o = V.op_order((a, b, c))
                counts[o] = counts.get(o, 0) + 1
    assert sorted(counts) == sorted(S.ORDERS) and set(counts.values()) == {12 ** 3 // 24}


def test_bad_records_raise():
    sizes = [(256, 341)]

    def rec(**kw):
        return V.view_records(sizes, S.params_of([S.plain_view(**kw)]))

    rec()
    for kw in (dict(top=40), dict(left=120), dict(top=-1), dict(h=0), dict(w=0, left=0), dict(ops=(0, 1, 2, 2)), dict(ops=(0, 1, 2, 4)), dict(sigma=0.05),
               dict(sigma=2.5), dict(sigma=float("nan")), dict(brightness=float("inf")), dict(hue=float("nan"))):
        with pytest.raises(ValueError):
            rec(**kw)
    with pytest.raises(ValueError):     # a box larger than the kernel's limit
        V.view_records([(4000, 4000)], S.params_of([S.plain_view(h=3585, w=3585)]))
    V.view_records([(4000, 4000)], S.params_of([S.plain_view(h=3584, w=3584)]))
    with pytest.raises(ValueError):     # a view that names no image
        V.view_records(sizes, S.params_of([S.plain_view()], image=[1]))
    with pytest.raises(ValueError):
        V.view_records(sizes, S.params_of([S.plain_view()]), offsets=[-4])
    with pytest.raises(ValueError):
        V.view_records([(70000, 10)], S.params_of([S.plain_view(h=10, w=10)]))


# ---- the oracle, pinned against independent sources ---------------------------------------------------------------------------------
def _hue_pixels():
    g = torch.Generator().manual_seed(5)
    special = torch.tensor([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0.2, 0.2, 0.2], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1],
                            [0.7, 0.7, 0.1], [0.3, 0.9, 0.9], [0.6, 0.2, 0.6], [0.4, 0.4, 0.39], [1e-3, 0, 0]], dtype=torch.float64)
    rnd = torch.rand(2000, 3, dtype=torch.float64, generator=g)
    u8 = torch.randint(0, 256, (2000, 3), generator=g).double() / 255      # many exact ties
    return torch.cat([special, rnd, u8])


def test_oracle_hue_is_colorsys_in_fp64():
    px = _hue_pixels()
    img = px.T.reshape(3, 1, -1).contiguous()
    worst = 0.0
    for f in (-0.2, -0.0731, 0.0, 0.2, 0.5, -0.5):
        got = S.hue(img, f).reshape(3, -1).T
        want = torch.tensor([colorsys.hsv_to_rgb(*((lambda h, s, v: ((h + f) % 1.0, s, v))(*colorsys.rgb_to_hsv(*p.tolist())))) for p in px], dtype=torch.float64)
        worst = max(worst, (got - want).abs().max().item())
    assert worst <= 1e-12, worst


def test_oracle_blends_are_image_enhance_within_2_lsb():
    """PIL truncates the blend (< 1 LSB) and rounds its degenerate image (<= 0.5 LSB, times |1 - f| <= 0.8): 2 / 255 bounds the gap."""
    from PIL import Image, ImageEnhance

    img = S.fixture_image(64, 96, seed=2)
    x = torch.from_numpy(img).permute(2, 0, 1).float() / 255
    im = Image.fromarray(img)
    worst = 0.0
    for f in (0.2, 0.63, 1.0, 1.37, 1.8):
        for ours, theirs in ((S.brightness, ImageEnhance.Brightness), (S.contrast, ImageEnhance.Contrast), (S.saturation, ImageEnhance.Color)):
            want = torch.from_numpy(np.array(theirs(im).enhance(f))).permute(2, 0, 1).float() / 255
            worst = max(worst, (ours(x, f) - want).abs().max().item())
    assert worst <= 2 / 255, worst


def test_oracle_blur_is_conv2d_on_a_reflect_padded_input():
    g = torch.Generator().manual_seed(8)
    x = torch.rand(3, 224, 224, dtype=torch.float64, generator=g)
    for sigma in (0.1, 0.5, 1.0, 2.0):
        w = S.gaussian_weights(sigma, torch.float64)
        k2 = (w[:, None] @ w[None, :]).expand(3, 1, 21, 21)
        want = F.conv2d(F.pad(x[None], (10, 10, 10, 10), mode="reflect"), k2, groups=3)[0]
        assert (S.blur(x, sigma) - want).abs().max().item() <= 1e-14, sigma
        assert abs(w.sum().item() - 1) < 1e-15 and torch.equal(w, w.flip(0))
    assert (S.blur(x.float(), 1.0).double() - S.blur(x, 1.0)).abs().max().item() < 1e-6


def test_float_path_against_the_pil_path_the_reference_runs():
    """Reference against reference, not the code under test: how far torchvision's float tensor path (what the kernel implements) stands
    from its PIL backend (what the reference's DataLoader runs) over the 24 orders on the seeded 256 x 341 fixture.  Measured here:
    max 0.0196 without hue; with hue max 0.1033 and mean 0.0124 (PIL's 8-bit hue on weakly saturated pixels); the gates are twice that."""
    img = S.fixture_image()
    mx = mn = mx_nohue = 0.0
    for v in S.gap_views():
        d = (S.float_view(img, v) - S.pil_view(img, v)).abs()
        mx, mn = max(mx, d.max().item()), max(mn, d.mean().item())
        v2 = dict(v, ops=tuple(o for o in v["ops"] if o != 3))
        mx_nohue = max(mx_nohue, (S.float_view(img, v2) - S.pil_view(img, v2)).abs().max().item())
    print(f"float path - PIL path: max {mx:.4f} mean {mn:.4f} with hue, max {mx_nohue:.4f} without")
    assert mx_nohue <= 2 * 0.0196 and mx <= 2 * 0.1033 and mn <= 2 * 0.0124, (mx_nohue, mx, mn)
    assert mx_nohue > 1e-3      # the two paths do differ: the comparison is not vacuous
