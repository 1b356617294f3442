"""Host side of the device image transforms (clibd_amd.augment): the size rules, the samplers against a restatement of torchvision's,
decode / pack, record validation, and the oracle's own conventions.  No GPU."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from clibd_amd import augment as A
from tests import augment_reference as R


def _encode(a: np.ndarray, fmt: str, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format=fmt, **kw)
    return buf.getvalue()


def _rgb(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("hw, want", [((400, 300), (341, 256)), ((300, 400), (256, 341)), ((500, 500), (256, 256)), ((256, 341), (256, 341)),
                                      ((256, 2000), (256, 2000)), ((2000, 256), (2000, 256)), ((683, 512), (341, 256)), ((10, 15), (256, 384))])
def test_resize_size_rule(hw, want):
    assert A.resize_size(*hw) == want


def test_center_crop_offsets_round_half_to_even():
    assert A.center_crop_offsets(256, 341) == (16, 58)      # (341 - 224) / 2 = 58.5 -> 58
    assert A.center_crop_offsets(256, 343) == (16, 60)      # 59.5 -> 60
    assert A.center_crop_offsets(225, 224) == (0, 0)        # 0.5 -> 0
    assert A.center_crop_offsets(227, 2000) == (2, 888)     # 1.5 -> 2


def test_params_from_uniforms_match_get_params():
    g = torch.Generator().manual_seed(3)
    sizes = [(256, 341), (341, 256), (256, 256), (256, 2000), (2000, 256), (300, 300), (10, 15), (1024, 1365), (257, 263)] * 40
    u = A.draw_uniforms(len(sizes), g)
    # forced fallbacks: every attempt asks for the whole area at the extreme ratios
    u[:9, :2 * A.ATTEMPTS] = 0.999999
    u[9:18, :2 * A.ATTEMPTS:2] = 0.999999
    u[9:18, 1:2 * A.ATTEMPTS:2] = 0.0
    p = A.params_from_uniforms(sizes, u)
    for i, (H0, W0) in enumerate(sizes):
        H1, W1 = A.resize_size(H0, W0)
        assert (p["H1"][i], p["W1"][i]) == (H1, W1)
        want = R.get_params(H1, W1, u[i].tolist())
        assert (p["top"][i], p["left"][i], p["h"][i], p["w"][i]) == want, (i, H0, W0)
    assert (p["h"][3], p["w"][3]) == (256, 341) and (p["h"][4], p["w"][4]) == (341, 256)    # fallback, ratio clamped
    assert (p["h"][2], p["w"][2]) == (256, 256) and p["top"][2] == 0                          # fallback, whole image
    assert (p["h"] <= A.CROP_MAX).all() and (p["w"] <= A.CROP_MAX).all()


def test_sampler_statistics():
    n = 100_000
    p = A.params_from_uniforms([(256, 341)] * n, A.draw_uniforms(n, torch.Generator().manual_seed(11)))
    assert abs(p["hflip"].mean() - 0.5) < 0.01 and abs(p["vflip"].mean() - 0.5) < 0.01
    assert -45.0 <= p["angle"].min() < -44.9 and 44.9 < p["angle"].max() <= 45.0
    frac = p["h"] * p["w"] / (256 * 341)
    assert 0.075 < frac.min() < 0.085 and 0.97 < frac.max() <= 1.0
    ratio = p["w"] / p["h"]
    assert ratio.min() > 0.73 and ratio.max() < 1.36


def test_sample_train_params_records():
    sizes = [(256, 341), (512, 683), (10, 15)]
    rec = A.sample_train_params(sizes, torch.Generator().manual_seed(0))
    assert rec.dtype == torch.int32 and rec.shape == (3, A.RECORD_INT32)
    r = rec.numpy().view(A._RECORD).reshape(-1)
    assert list(r["offset"]) == [0, 256 * 341 * 3, 256 * 341 * 3 + 512 * 683 * 3]
    assert list(r["H1"]) == [256, 256, 256] and list(r["W1"]) == [341, 341, 384]
    assert (r["flags"] & A.FLAG_ROTATE).all()
    p = A.params_from_uniforms(sizes, A.draw_uniforms(3, torch.Generator().manual_seed(0)))
    for i in range(3):
        np.testing.assert_array_equal(r["theta"][i], A.rotation_theta(float(p["angle"][i])))
        assert (r["top"][i], r["left"][i], r["h"][i], r["w"][i]) == (p["top"][i], p["left"][i], p["h"][i], p["w"][i])
        assert r["flags"][i] == A.FLAG_ROTATE | (A.FLAG_HFLIP if p["hflip"][i] else 0) | (A.FLAG_VFLIP if p["vflip"][i] else 0)
    # the same draw again is the same record; eval records are centre crops without flags
    assert torch.equal(rec, A.sample_train_params(sizes, torch.Generator().manual_seed(0)))
    e = A.eval_params(sizes).numpy().view(A._RECORD).reshape(-1)
    assert list(e["top"]) == [16, 16, 16] and list(e["left"]) == [58, 58, 80] and (e["h"] == 224).all() and (e["flags"] == 0).all()


def test_rotation_theta_convention():
    t = A.rotation_theta(30.0)
    a = np.radians(30.0)
    np.testing.assert_array_equal(t, np.array([np.cos(a), -np.sin(a), 0, np.sin(a), np.cos(a), 0], dtype=np.float64).astype(np.float32))
    assert t.dtype == np.float32


def test_oracle_quarter_turns_are_rot90():
    x = torch.rand(3, 224, 224, generator=torch.Generator().manual_seed(0))
    assert torch.equal(R.rotate(x, 90.0), torch.rot90(x, 1, (-2, -1)))
    assert torch.equal(R.rotate(x, -90.0), torch.rot90(x, -1, (-2, -1)))
    assert torch.equal(R.rotate(x, 0.0), x)


@pytest.mark.parametrize("fmt", ["JPEG", "PNG"])
def test_decode_pack_equals_pil(fmt):
    imgs = [_rgb(37, 53, 1), _rgb(256, 341, 2), _rgb(5, 3, 3)]
    enc = [_encode(a, fmt) for a in imgs]
    data, offsets, sizes = A.decode_images(enc, threads=3, pin=False)
    assert sizes.tolist() == [[37, 53], [256, 341], [5, 3]]
    assert offsets.tolist() == [0, 37 * 53 * 3, 37 * 53 * 3 + 256 * 341 * 3, 37 * 53 * 3 + 256 * 341 * 3 + 45]
    for i, e in enumerate(enc):
        want = np.asarray(Image.open(io.BytesIO(e)))
        got = data[offsets[i]:offsets[i + 1]].numpy().reshape(want.shape)
        np.testing.assert_array_equal(got, want)
    # the reference's HDF5 layout: zero-padded rows + lengths
    L = max(len(e) for e in enc)
    pad = np.zeros((len(enc), L + 7), dtype=np.uint8)
    for i, e in enumerate(enc):
        pad[i, :len(e)] = np.frombuffer(e, dtype=np.uint8)
    d2, o2, s2 = A.decode_images(torch.from_numpy(pad), lengths=[len(e) for e in enc], pin=False)
    assert torch.equal(d2, data) and torch.equal(o2, offsets) and torch.equal(s2, sizes)


def test_default_threads_capped():
    assert 1 <= A.default_threads() <= 16


def test_bad_inputs_raise():
    gray = _encode(np.zeros((8, 8), np.uint8), "PNG")
    rgba = _encode(np.zeros((8, 8, 4), np.uint8), "PNG")
    ok = _encode(_rgb(8, 8), "PNG")
    for bad in ([gray], [rgba], [ok, b""], []):
        with pytest.raises(ValueError):
            A.decode_images(bad, pin=False)
    with pytest.raises(ValueError):
        A.decode_images(np.zeros((2, 4), np.uint8), lengths=[1, 5], pin=False)
    with pytest.raises(ValueError):
        A.eval_params([(0, 10)])
    with pytest.raises(ValueError):
        A.eval_params([(5000, 6000)])            # short side beyond the kernel's 16x downscale
    p = A.params_from_uniforms([(256, 341)], A.draw_uniforms(1, torch.Generator().manual_seed(0)))
    for k, v in (("top", 300), ("left", -1), ("h", 0), ("w", 400)):
        q = dict(p)
        q[k] = np.array([v])
        with pytest.raises(ValueError):
            A.train_records([(256, 341)], q)
    with pytest.raises(ValueError):
        A.eval_params([(256, 341)], offsets=[-3])


def test_collate_encoded_structure():
    samples = [(f"p{i}", _encode(_rgb(30 + i, 40, i), "JPEG"), torch.arange(5) + i, torch.zeros(20, dtype=torch.long), torch.zeros(20, dtype=torch.long),
                torch.ones(20, dtype=torch.long), i) for i in range(3)]
    pid, image, dna, ids, tt, am, label = A.collate_encoded(samples, train=True, generator=torch.Generator().manual_seed(0), threads=2)
    assert pid == ["p0", "p1", "p2"] and A.is_packed(image)
    assert image["data"].dtype == torch.uint8 and image["offsets"].tolist()[-1] == image["data"].numel()
    assert image["xforms"].shape == (3, A.RECORD_INT32) and dna.shape == (3, 5) and label.tolist() == [0, 1, 2]
    ev = [s[:6] + ({"order": "o", "family": "f", "genus": "g", "species": f"s{i}"},) for i, s in enumerate(samples)]
    out = A.collate_encoded(ev, train=False)
    assert out[6]["species"] == ["s0", "s1", "s2"] and (out[1]["xforms"].numpy().view(A._RECORD)["flags"] == 0).all()


def test_augment_kernels_use_no_scratch():
    from clibd_amd import build

    rows = [(k["name"], k["scratch"]) for k in build.resource_usage("augment")]
    assert len(rows) == 3, rows
    assert all(s == 0 for _, s in rows), rows
