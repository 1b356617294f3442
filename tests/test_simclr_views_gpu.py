"""clibd_simclr_views_u8 (csrc/views.hip) through clibd_amd.simclr_views / ops.simclr_views against the torch restatement of torchvision's
float tensor path (tests/simclr_views_reference.py), and the packed-batch form of SimCLR.train_step.

Gate of the oracle comparisons: the oracle is evaluated in fp32 and in fp64 on the test's own inputs; the kernel must stand within
8 x the largest gap between the two (its summation order, expf and divisions differ from the fp32 oracle's), never below 1e-5, the gate
of the resample comparison in tests/test_augment_gpu.py.  The comparison is against the fp64 values."""
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clibd_amd import augment as A
from clibd_amd import ops
from clibd_amd import simclr_views as V
from tests import simclr_views_reference as S

pytestmark = pytest.mark.gpu


def _run(imgs, views, image, dev):
    """the kernel's views [n, 3, 224, 224] (on the CPU) of view dicts over the images `image` names"""
    sizes = np.array([a.shape[:2] for a in imgs], dtype=np.int64)
    rec = V.view_records(sizes, S.params_of(views, image))
    data = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs]))
    return ops.simclr_views(data.to(dev), rec.to(dev)).cpu()


def _oracle(imgs, views, image):
    """(fp64 views, gate): gate = max(8 x max |fp32 oracle - fp64 oracle|, 1e-5)"""
    ref = [S.float_view(imgs[i], v, torch.float64) for v, i in zip(views, image)]
    gap = max((S.float_view(imgs[i], v, torch.float32).double() - r).abs().max().item() for v, i, r in zip(views, image, ref))
    return ref, max(8 * gap, 1e-5), gap


def _check(out, ref, gate, what):
    errs = [(o.double() - r).abs().max().item() for o, r in zip(out, ref)]
    print(f"{what}: max error {max(errs):.3e}, gate {gate:.3e}")
    assert max(errs) <= gate, (what, errs, gate)
    return max(errs)


def _hue_fixture() -> np.ndarray:
    """224 x 224: noise, plus rows of grays, black, white, the primaries and their pairs, and pixels whose two largest channels tie"""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (224, 224, 3)).astype(np.uint8)
    a[0:8] = np.arange(224, dtype=np.uint8)[None, :, None]                       # grays, black included
    a[8:12] = 0
    a[12:16] = 255
    for k, c in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (128, 0, 0), (0, 7, 0)]):
        a[16 + 2 * k:18 + 2 * k] = c
    t = rng.integers(0, 256, (3, 224)).astype(np.uint8)
    a[32:36, :, 0], a[32:36, :, 1], a[32:36, :, 2] = t[0], t[0], np.minimum(t[0], t[1])     # r == g >= b
    a[36:40, :, 0], a[36:40, :, 1], a[36:40, :, 2] = np.minimum(t[0], t[1]), t[0], t[0]     # g == b >= r
    a[40:44, :, 0], a[40:44, :, 1], a[40:44, :, 2] = t[2], np.minimum(t[2], t[1]), t[2]     # r == b >= g
    return a


def test_identity_record_is_an_exact_copy(dev):
    """A 224 x 224 box, no flip, no jitter, no gray, sigma 0.1: the neighbouring blur weights are exp(-50) = 2e-22 of the centre's and vanish
    beside any pixel >= 1 / 255, so the output is u8 / 255 exactly.  (Beside an exactly black pixel the neighbours' 2e-22 is all there is, in
    torch's convolution as well: the fixture has no zero byte.)"""
    rng = np.random.default_rng(0)
    imgs = [rng.integers(1, 256, (224, 224, 3)).astype(np.uint8), rng.integers(1, 256, (256, 341, 3)).astype(np.uint8)]
    out = _run(imgs, [S.plain_view(), S.plain_view(top=17, left=101)], [0, 1], dev)
    assert torch.equal(out[0], torch.from_numpy(imgs[0]).permute(2, 0, 1).float() / 255)
    assert torch.equal(out[1], torch.from_numpy(imgs[1][17:241, 101:325]).permute(2, 0, 1).float() / 255)


def test_each_colour_operation_alone(dev):
    """One operation away from neutral at a time (the other factors 1, 1, 1, 0; blend at factor 1 is exact)."""
    imgs = [S.fixture_image(224, 224, seed=1), _hue_fixture()]
    cases = [("brightness", 1.8, 0), ("contrast", 0.2, 0), ("contrast", 1.8, 0), ("saturation", 0.2, 0), ("saturation", 1.8, 0), ("hue", 0.2, 1), ("hue", -0.2, 1),
             ("saturation", 1.8, 1), ("contrast", 1.8, 1)]
    views = [S.plain_view(jitter=True, **{k: f}) for k, f, _ in cases]
    image = [i for _, _, i in cases]
    assert (S.brightness(torch.from_numpy(imgs[0]).float() / 255, 1.8) == 1).float().mean() > 0.05      # brightness 1.8 saturates
    out = _run(imgs, views, image, dev)
    ref, gate, _ = _oracle(imgs, views, image)
    for k, (name, f, i) in enumerate(cases):
        _check(out[k:k + 1], ref[k:k + 1], gate, f"{name} {f} on image {i}")
        assert (ref[k] - torch.from_numpy(imgs[i]).permute(2, 0, 1).double() / 255).abs().max() > 0.05     # the operation did something


def test_all_24_orders_in_one_call(dev):
    """All four operations on, every order, sampler boxes and flips on the 256 x 341 fixture.  The contrast mean depends on the operations
    that precede it: taken at another stage it misses the gate by orders of magnitude."""
    img = S.fixture_image()
    views = S.gap_views()
    assert len(views) == 24 and sorted(v["ops"] for v in views) == sorted(S.ORDERS)
    out = _run([img], views, [0] * 24, dev)
    ref, gate, gap = _oracle([img], views, [0] * 24)
    _check(out, ref, gate, f"24 orders (oracle fp32-fp64 gap {gap:.3e})")
    # the check is sharp: with the mean of the image as it ENTERS the chain, the orders that have contrast last end elsewhere
    off = []
    for k, v in enumerate(views):
        if v["ops"][3] == 1:
            x = wrong = S.crop_resample(img, v, torch.float64)
            for op in v["ops"]:
                wrong = S.blend(wrong, S.gray_of(x).mean(), v["contrast"]) if op == 1 else S.colour_ops(wrong, dict(v, ops=(op,)))
            off.append((S.blur(wrong, v["sigma"]) - ref[k]).abs().max().item())
    assert len(off) == 6 and max(off) > 100 * gate, (off, gate)


def test_gray_flag(dev):
    img = S.fixture_image()
    p = V.params_from_uniforms([(256, 341)] * 2, V.draw_view_uniforms(2, torch.Generator().manual_seed(21)))
    views = [dict(S.view_of(p, r), gray=True, jitter=r % 2 == 0) for r in range(4)]
    out = _run([img], views, [0] * 4, dev)
    for o in out:
        assert torch.equal(o[0], o[1]) and torch.equal(o[0], o[2])
    ref, gate, _ = _oracle([img], views, [0] * 4)
    _check(out, ref, gate, "gray")


def test_blur_and_its_reflect_padding(dev):
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, (224, 224, 3)).astype(np.uint8)
    imp = np.zeros((224, 224, 3), dtype=np.uint8)
    for y, x in ((0, 0), (0, 223), (223, 223), (112, 0), (223, 100), (60, 60)):
        imp[y, x] = 255
    sigmas = (0.1, 0.5, 1.0, 2.0)
    views = [S.plain_view(sigma=s) for s in sigmas] * 2
    image = [0] * 4 + [1] * 4
    out = _run([noise, imp], views, image, dev)
    ref, gate, _ = _oracle([noise, imp], views, image)
    border = torch.zeros(224, 224, dtype=torch.bool)
    border[:10], border[-10:], border[:, :10], border[:, -10:] = True, True, True, True
    for k in range(8):
        d = (out[k].double() - ref[k]).abs()
        eb, ei = d[:, border].max().item(), d[:, ~border].max().item()
        print(f"blur sigma {views[k]['sigma']} image {image[k]}: border {eb:.3e} interior {ei:.3e} gate {gate:.3e}")
        assert eb <= gate and ei <= gate, (k, eb, ei, gate)
    # zero or replicate padding would show in the outer ten rows and columns
    x = torch.from_numpy(noise).permute(2, 0, 1).double() / 255
    w = S.gaussian_weights(2.0, torch.float64)
    k2 = (w[:, None] @ w[None, :]).expand(3, 1, 21, 21)
    for mode in ("replicate", "constant"):
        other = F.conv2d(F.pad(x[None], (10, 10, 10, 10), mode=mode), k2, groups=3)[0]
        assert (other - ref[3])[:, border].abs().max().item() > 100 * gate and (other - ref[3])[:, ~border].abs().max().item() < 1e-12


GEOM_SIZES = [(224, 224), (256, 341), (37, 53), (600, 800)]


def test_geometry_matches_the_dataset_transform(dev):
    """Jitter and gray off, sigma 0.1: the sampler's boxes and flips give what ops.image_transform gives for the matching record (H1 = H0,
    W1 = W0, no rotation) within 1e-5, and the oracle's crop.  Boxes beyond that entry's 384 limit (the 500 x 640 one, the whole 600 x 800
    image) are only this entry's: they are compared with the oracle alone."""
    imgs = [S.fixture_image(h, w, seed=h) for h, w in GEOM_SIZES]
    sizes = GEOM_SIZES * 3
    p = V.params_from_uniforms(sizes, V.draw_view_uniforms(len(sizes), torch.Generator().manual_seed(31)))
    views = [dict(S.view_of(p, r), jitter=False, gray=False, sigma=0.1) for r in range(2 * len(sizes))]
    image = [int(i) % 4 for i in p["image"]]
    views += [S.plain_view(top=50, left=80, h=500, w=640), S.plain_view(top=0, left=0, h=600, w=800, hflip=True), S.plain_view(top=0, left=0, h=37, w=53),
              S.plain_view(top=3, left=5, h=30, w=40, hflip=True), S.plain_view(top=0, left=0, h=256, w=341)]
    image += [3, 3, 2, 2, 1]
    assert any(v["hflip"] for v in views[:24]) and any(not v["hflip"] for v in views[:24])
    out = _run(imgs, views, image, dev)
    ref, gate, _ = _oracle(imgs, views, image)
    _check(out, ref, gate, "geometry against the oracle")
    small = [k for k, v in enumerate(views) if v["h"] <= A.CROP_MAX and v["w"] <= A.CROP_MAX]
    assert len(small) >= 20 and len(small) < len(views)
    isz = np.array(GEOM_SIZES, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(isz[:, 0] * isz[:, 1] * 3)])
    q = {k: np.array([views[j][k] for j in small]) for k in ("top", "left", "h", "w", "hflip")}
    q["vflip"] = np.zeros(len(small), dtype=bool)
    s1 = isz[[image[j] for j in small]]
    q["H1"], q["W1"] = s1[:, 0], s1[:, 1]
    rec = A.train_records(s1, q, offsets=offs[[image[j] for j in small]], rotate=False)
    data = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs]))
    want = ops.image_transform(data.to(dev), rec.to(dev)).cpu()
    err = (out[small] - want).abs().max().item()
    print(f"geometry against image_transform: {err:.3e}")
    assert err <= 1e-5, err


def test_device_guard_gives_a_zero_image_and_reads_nothing_outside(dev):
    """Records the host would refuse, written into the tensor behind its back: each yields a zero image and its neighbours stay right.
    `data` is over-allocated so that even an unguarded read of the oversized box would stay inside the allocation."""
    img = S.fixture_image()
    views = [dict(v, jitter=True) for v in S.gap_views()[:7]]
    rec = V.view_records([(256, 341)], S.params_of(views, [0] * 7))
    good = rec.clone()
    r = rec.numpy().view(V._RECORD).reshape(-1)
    r["h"][1] = 256 + 50                            # the box leaves the image
    r["top"][1] = 0
    r["order"][2] = V.pack_order((0, 1, 2, 2))      # not a permutation
    r["sigma"][3] = 3.0
    r["contrast"][4] = np.float32("nan")
    r["offset"][5] = img.size * 4 + 1               # the pixels end one byte outside data
    full = torch.from_numpy(np.concatenate([img.reshape(-1), np.zeros(img.size * 4 + 4096, dtype=np.uint8)])).to(dev)
    data = full[:img.size * 5]                      # what the entry is told; the allocation goes on
    out = ops.simclr_views(data, rec.to(dev)).cpu()
    want = ops.simclr_views(data, good.to(dev)).cpu()
    for k in (1, 2, 3, 4, 5):
        assert (out[k] == 0).all() and want[k].abs().max() > 0, k
    for k in (0, 6):
        assert torch.equal(out[k], want[k]), k
    ref, gate, _ = _oracle([img], [views[0], views[6]], [0, 0])
    _check(out[[0, 6]], ref, gate, "neighbours of the bad records")


def test_independence_and_repeatability(dev):
    imgs = [S.fixture_image(), S.fixture_image(600, 800, seed=5), S.fixture_image(37, 53, seed=6)]
    vs = S.gap_views()
    views, image = [vs[1], vs[7], dict(vs[13], top=2, left=3, h=30, w=45), vs[3], vs[20]], [1, 0, 2, 0, 1]
    a = _run(imgs, views, image, dev)
    assert torch.equal(a, _run(imgs, views, image, dev))
    alone = _run([imgs[0]], [views[3]], [0], dev)         # the same image and record alone, at offset 0
    assert torch.equal(alone[0], a[3])


def _jpegs(sizes, seed):
    from PIL import Image

    enc = []
    for k, (h, w) in enumerate(sizes):
        buf = io.BytesIO()
        Image.fromarray(S.fixture_image(h, w, seed=seed + k)).save(buf, format="JPEG", quality=90)
        enc.append(buf.getvalue())
    return enc


def _decoded(enc):
    from PIL import Image

    return [np.asarray(Image.open(io.BytesIO(e))) for e in enc]


def test_packed_batch_layout(dev):
    """apply(pack_two_views(...)): row i and row B + i are views of sample i, both read the same bytes."""
    enc = _jpegs([(256, 341), (300, 280), (224, 224), (120, 90)], 40)
    B = len(enc)
    packed = V.collate_two_views(enc, torch.Generator().manual_seed(2))
    assert sorted(packed) == ["data", "offsets", "xforms"] and tuple(packed["xforms"].shape) == (2 * B, 16)
    assert torch.equal(packed["xforms"], V.pack_two_views(enc, torch.Generator().manual_seed(2))["xforms"])
    r = packed["xforms"].numpy().view(V._RECORD).reshape(-1)
    assert np.array_equal(r["offset"][:B], packed["offsets"][:-1].numpy()) and np.array_equal(r["offset"][B:], r["offset"][:B])
    out = V.apply(packed, dev).cpu()
    assert tuple(out.shape) == (2 * B, 3, 224, 224)
    imgs = _decoded(enc)
    views = S.views_of_records(packed["xforms"])
    image = list(range(B)) * 2
    ref, gate, _ = _oracle(imgs, views, image)
    _check(out, ref, gate, "packed batch")
    assert not torch.equal(out[0], out[B])


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.flat = torch.nn.Flatten()
        self.lin = torch.nn.Linear(3 * 224 * 224, 8)

    def forward(self, x):
        return self.lin(self.flat(x))


def _args():
    import types

    mc = types.SimpleNamespace(temperature=0.07, n_views=2, batch_size=4, epochs=1, model_output_name="simclr_views_test", image=types.SimpleNamespace())
    return types.SimpleNamespace(model_config=mc, project_root_path=".")


def test_step_from_a_packed_batch(dev, tmp_path):
    from clibd_amd.model import create_vit
    from clibd_amd.optim import FusedAdam
    from clibd_amd.simclr import SimCLR, SimCLRViT

    enc = _jpegs([(256, 341), (300, 280), (224, 224), (120, 90)], 50)
    packed = V.pack_two_views(enc, torch.Generator().manual_seed(9))
    views = V.apply(packed, dev).clone()
    losses = []
    for form in ("packed", "tensors"):
        torch.manual_seed(0)
        model = _Stub()
        sim = SimCLR(model=model, optimizer=torch.optim.SGD(model.parameters(), lr=0.1), scheduler=None, device=dev, args=_args())
        w0 = model.lin.weight.detach().clone()
        loss = sim.train_step(packed) if form == "packed" else sim.train_step(views[:4], views[4:])
        losses.append((loss.clone(), model.lin.weight.detach().clone()))
        assert (losses[-1][1] - w0).abs().max().item() > 0
    assert torch.equal(losses[0][0], losses[1][0]), (losses[0][0].item(), losses[1][0].item())
    with pytest.raises(ValueError):
        sim.train_step(packed, views[4:])
    # a loader that yields packed batches
    best = sim.train([packed, V.pack_two_views(enc, torch.Generator().manual_seed(10))], rank=0, ckpt_dir=str(tmp_path))
    assert best == best and (tmp_path / "checkpoint_0001.pth.tar").exists()

    # the smallest ViT that tests/test_simclr_gpu.py trains, fed from the packed batch
    torch.manual_seed(3)
    model = SimCLRViT(create_vit("vit_small_patch16_224", num_classes=1000, depth=2)).to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    sim = SimCLR(model=model, optimizer=FusedAdam(model.parameters(), lr=3e-4, weight_decay=1e-4), scheduler=None, device=dev, args=_args())
    loss = sim.train_step(packed)
    assert torch.isfinite(loss).item() and loss.item() > 0
