"""Device JPEG decode against PIL on an MI355X: `decode_images_device` equals `decode_images` byte for byte over the corpus of
tests/jpeg_corpus.py (as one batch and class by class), in both input layouts and in mixed batches; `apply` on a
`collate_encoded(decode="device")` batch equals `apply` on the host-decoded one; the damage set that the stand-alone host program of
tests/test_jpeg_cpu.py decodes under the sanitizers leaves 4 KiB guard bands untouched, every good image equal to PIL's and every
truncated stream with a status and a zero slice; two runs, and a batch of one, give the same bytes.  Every comparison with PIL also asserts
that the device's status of every eligible member is 0: `decode_images_device` decodes again on the host whatever the device stopped on,
so equal pixels alone would not show a kernel that gives up.  The damage set reaches the GPU only through the fixture `sanitized`, which
first builds tests/jpeg_fetch_main.cpp under AddressSanitizer and UBSan and runs it over the same set on the host."""
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import jpeg_corpus as JC  # noqa: E402
from clibd_amd import augment as A  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096
CLASSES = [f"{s}-{o}" for s in ("444", "422", "420") for o in JC.OPTIONS]


@pytest.fixture(scope="module")
def host_reference():
    """(data, offsets, sizes) of `decode_images` over the whole eligible corpus: computed once, never modified"""
    return A.decode_images([e[5] for e in JC.eligible()], pin=False)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """The gate in front of the damage set: jpeg_core.h, the code the entropy kernel is compiled from, built as a host program with
    -fsanitize=address,undefined and run over JC.damaged() from buffers of exactly each stream's size.  Unless it ends clean (and reports
    every truncation) the tests that use this fixture fail here, before any malformed stream is launched on the GPU."""
    d = tmp_path_factory.mktemp("jpeg_gate")
    dm = JC.damaged()
    got = JC.run_program(JC.build_program(d), d, [(x[0], x[2]) for x in dm])
    for (name, kind, _), (reason, status) in zip(dm, got):
        if kind in ("truncated", "no_eoi", "rst_removed", "rst_duplicated"):
            assert reason == 0 and status >= 32, (name, reason, status)
    return dm


def _same(got, want, names, decoded_on_device=None):
    """pixels, offsets and sizes equal to the host's; decoded_on_device: which members the device must have finished itself (default: all)"""
    data, offsets, sizes, status = got
    want_dev = np.ones(len(names), dtype=bool) if decoded_on_device is None else np.asarray(decoded_on_device)
    stopped = [(names[i], int(status[i])) for i in np.nonzero(want_dev)[0] if int(status[i]) != 0]
    assert not stopped, f"{len(stopped)} of {int(want_dev.sum())} eligible images were not decoded on the device (name, status): {stopped[:12]}"
    assert torch.equal(offsets, want[1]) and torch.equal(sizes, want[2])
    d, w, off = data.cpu(), want[0], want[1].tolist()
    if not torch.equal(d, w):
        bad = [names[i] for i in range(len(names)) if not torch.equal(d[off[i]:off[i + 1]], w[off[i]:off[i + 1]])]
        raise AssertionError(f"{len(bad)} of {len(names)} images differ from PIL's: {bad[:12]}")


# ---- pixel equality -------------------------------------------------------------------------------------------------------------------
def test_whole_corpus_in_one_batch_equals_pil(dev, host_reference):
    el = JC.eligible()
    got = A.decode_images_device([e[5] for e in el], device=dev, return_status=True)
    assert got[0].is_cuda and got[0].dtype == torch.uint8
    _same(got, host_reference, [e[0] for e in el])


@pytest.mark.parametrize("cls", CLASSES)
def test_each_class_equals_pil(dev, host_reference, cls):
    el = JC.eligible()
    idx = [i for i, e in enumerate(el) if e[1] == cls]
    assert len(idx) >= 42
    off = host_reference[1].tolist()
    want_data = torch.cat([host_reference[0][off[i]:off[i + 1]] for i in idx])
    sizes = host_reference[2][idx]
    want = (want_data, torch.from_numpy(A._packed_offsets(sizes.numpy())), sizes)
    _same(A.decode_images_device([el[i][5] for i in idx], device=dev, return_status=True), want, [el[i][0] for i in idx])


def test_hdf5_layout_equals_list_layout(dev):
    enc = [e[5] for e in JC.eligible() if e[2:4] in ((17, 23), (64, 48)) and "-q75-" in e[0]]
    lmax = max(len(e) for e in enc) + 5
    image = np.zeros((len(enc), lmax), dtype=np.uint8)
    for i, e in enumerate(enc):
        image[i, :len(e)] = np.frombuffer(e, dtype=np.uint8)
    lens = np.array([len(e) for e in enc])
    a = A.decode_images_device(enc, device=dev, return_status=True)
    for args in ((image, lens), (torch.from_numpy(image), torch.from_numpy(lens))):
        b = A.decode_images_device(args[0], lengths=args[1], device=dev, return_status=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and not b[3].any()
    _same(a, A.decode_images(image, lengths=lens, pin=False), [str(i) for i in range(len(enc))])


def test_mixed_batch_equals_host_and_modes_raise(dev):
    ne = JC.not_eligible()
    el = [e[5] for e in JC.eligible() if e[2:4] == (33, 47) and "-q5-" in e[0]][:6]
    enc = [ne["png"], el[0], el[1], ne["progressive"], el[2], ne["progressive"], el[3], ne["png"]]
    on_device = [False, True, True, False, True, False, True, False]
    got = A.decode_images_device(enc, device=dev, return_status=True)
    _same(got, A.decode_images(enc, pin=False), [str(i) for i in range(len(enc))], on_device)
    assert got[3].tolist() == [1, 0, 0, 3, 0, 3, 0, 1]                 # the plan's reason where the host decoded from the start
    only_host = [ne["png"], ne["progressive"]]
    _same(A.decode_images_device(only_host, device=dev, return_status=True), A.decode_images(only_host, pin=False), ["png", "progressive"],
          [False, False])
    for mode, name in (("L", "gray"), ("CMYK", "cmyk")):
        with pytest.raises(ValueError, match=f"decode_images: {mode} image \\(the model takes RGB\\)"):
            A.decode_images_device([el[0], ne[name]], device=dev)


# ---- through the transforms -------------------------------------------------------------------------------------------------------------
def _samples(encoded):
    return [(f"p{i}", e, torch.arange(5) + i, torch.zeros(20, dtype=torch.long), torch.zeros(20, dtype=torch.long), torch.ones(20, dtype=torch.long), i)
            for i, e in enumerate(encoded)]


def test_apply_equals_the_host_decoded_batch(dev):
    from clibd_amd import simclr_views as V

    ne = JC.not_eligible()
    enc = [e[5] for e in JC.eligible() if e[2:4] in ((64, 48), (33, 47), (256, 341)) and ("-q75-" in e[0] or e[2] == 256)]
    enc = enc[:20] + [ne["png"]] + enc[-3:] + [ne["progressive"]]
    for train in (True, False):
        host = A.collate_encoded(_samples(enc), train, torch.Generator().manual_seed(11))
        devb = A.collate_encoded(_samples(enc), train, torch.Generator().manual_seed(11), decode="device")
        a, b = A.apply(host[1], dev), A.apply(devb[1], dev)
        assert a.shape == (len(enc), 3, 224, 224) and torch.equal(a, b)
        data, status = A.decode_packed(devb[1], dev, return_status=True)   # what `apply` ran: the device finished every eligible member
        assert status.tolist() == [0] * 20 + [1] + [0] * 3 + [3] and torch.equal(data.cpu(), host[1]["data"])
        moved = {k: v.to(dev) for k, v in devb[1].items()}             # as a prefetcher leaves the batch
        assert torch.equal(A.apply(moved), a)
    h = V.collate_two_views(enc, torch.Generator().manual_seed(12))
    d = V.collate_two_views(enc, torch.Generator().manual_seed(12), decode="device")
    a, b = V.apply(h, dev), V.apply(d, dev)
    assert a.shape == (2 * len(enc), 3, 224, 224) and torch.equal(a, b)
    assert A.decode_packed(d, dev, return_status=True)[1].tolist() == [0] * 20 + [1] + [0] * 3 + [3]


def test_out_of_range_images_are_handed_to_the_host(dev):
    """the CLIBD_JPEG_RANGE route on purpose, from both places that raise it (tests/jpeg_corpus.py::out_of_range): the device reports 37,
    the caller decodes the image with PIL, and the neighbours in the batch are decoded on the device as usual"""
    from clibd_amd import ops

    r = JC.out_of_range()
    good = [e[5] for e in JC.eligible() if e[2:4] == (16, 16) and "-q75-plain" in e[0]][:3]
    enc = [good[0], r["idct"], good[1], r["entropy"], good[2]]
    got = A.decode_images_device(enc, device=dev, return_status=True)
    assert got[3].tolist() == [0, 37, 0, 37, 0]
    _same(got, A.decode_images(enc, pin=False), ["good0", "idct", "good1", "entropy", "good2"], [True, False, True, False, True])
    packed, _ = A._pack_device(enc)                                   # and underneath: the flagged slices are zero, not half written
    out = torch.full((int(packed["offsets"][-1]),), 0xA5, dtype=torch.uint8, device=dev)
    head = packed["plans"][:, :56].contiguous().numpy().view(A._PLAN_HEAD).reshape(-1)
    assert (head["reason"] == 0).all()
    status = ops.jpeg_decode(packed["jpeg"].to(dev), packed["plans"].to(dev), packed["offsets"].to(dev), out, int(head["blocks"].sum()))
    off = packed["offsets"].tolist()
    assert status.tolist() == [0, 37, 0, 37, 0] and not out[off[1]:off[2]].any() and not out[off[3]:off[4]].any()
    assert torch.equal(out[off[2]:off[3]].cpu(), A.decode_images([good[1]], pin=False)[0])


def test_more_than_one_image_per_wave(dev):
    """B > 8192 is where the entropy kernel puts 2, 4 or 8 images into one workgroup (LDS slots, lane = slot): 8193 and 16500 tiny
    streams, twelve distinct ones in turn, so a slot that read its neighbour's record or stream would show"""
    el = [e for e in JC.eligible() if e[2:4] in ((1, 1), (7, 9)) and "-q75-" in e[0] and "-smooth-" in e[0]]
    assert len(el) == 24
    el = el[::2]
    ref = [torch.from_numpy(A._decode_one(e[5]).reshape(-1).copy()) for e in el]
    for B in (8193, 16500):
        pick = [(7 * i) % len(el) for i in range(B)]
        data, offsets, sizes, status = A.decode_images_device([el[k][5] for k in pick], device=dev, return_status=True)
        assert not status.any() and sizes.tolist() == [list(el[k][2:4]) for k in pick]
        assert torch.equal(data.cpu(), torch.cat([ref[k] for k in pick]))


# ---- the damage set -----------------------------------------------------------------------------------------------------------------------
def test_damaged_streams_stay_inside_their_buffers(dev, sanitized):
    from clibd_amd import ops

    good = [e for e in JC.eligible() if e[2:4] == (33, 47) and "-q100-" in e[0]]
    dm = [d for d in sanitized if d[1] != "bad_dht"]
    bufs, kinds = [], []
    for i, d in enumerate(dm):                                        # good and damaged interleaved
        bufs += [good[i % len(good)][5], d[2]]
        kinds += ["good", d[1]]
    B = len(bufs)
    plans = A.plan_streams(bufs)
    assert (plans["reason"] == 0).all()
    lens = np.array([len(b) for b in bufs])
    plans["stream_begin"] = np.concatenate([[0], np.cumsum(lens)])[:B]
    plans["coef_begin"] = np.concatenate([[0], np.cumsum(plans["blocks"].astype(np.int64))])[:B]
    nbytes = 3 * plans["H"].astype(np.int64) * plans["W"]
    offsets = GUARD + np.concatenate([[0], np.cumsum(nbytes + GUARD)])
    out = torch.full((int(offsets[-1]),), 0xA5, dtype=torch.uint8, device=dev)
    streams = torch.from_numpy(np.frombuffer(b"".join(bufs), dtype=np.uint8).copy()).to(dev)
    status = ops.jpeg_decode(streams, torch.from_numpy(plans.view(np.uint8).reshape(B, 4096)).to(dev), torch.from_numpy(offsets).to(dev), out,
                             int(plans["blocks"].sum())).cpu().numpy()
    got = out.cpu().numpy()
    at = 0
    for i in range(B):                                                # the guard bands before, between and after
        assert (got[at:offsets[i]] == 0xA5).all(), i
        at = offsets[i] + nbytes[i]
    assert (got[at:] == 0xA5).all() and len(got) - at == GUARD
    for i in range(B):
        sl = got[offsets[i]:offsets[i] + nbytes[i]]
        if kinds[i] == "good":
            assert status[i] == 0 and np.array_equal(sl, A._decode_one(bufs[i]).reshape(-1)), i
        elif kinds[i] in ("truncated", "no_eoi", "rst_removed", "rst_duplicated"):
            assert status[i] >= 32 and not sl.any(), (i, kinds[i], status[i])
        elif status[i] != 0:
            assert not sl.any(), i
    assert (status[np.array(kinds) == "flipped"] == 0).sum() >= 100   # most single-bit flips decode: those are compared with PIL below


def test_damaged_members_behave_as_on_the_host_path(dev, sanitized):
    """`apply` (and `decode_images_device`, which runs the same decode) on a damaged member: PIL's exception, or PIL's pixels"""
    good = [e[5] for e in JC.eligible() if e[2:4] == (33, 47) and "-q100-" in e[0]][:2]
    raises, decodes = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, kind, data in sanitized:
            try:
                A._decode_one(data)
                decodes.append((name, data))
            except Exception as e:  # noqa: BLE001
                raises.append((name, data, e))
        assert len(raises) >= 36 and len(decodes) >= 100
        enc = [good[0]] + [d for _, d in decodes] + [good[1]]
        names = ["good0"] + [n for n, _ in decodes] + ["good1"]
        _same(A.decode_images_device(enc, device=dev, return_status=True), A.decode_images(enc, pin=False), names,
              [True] + [False] * len(decodes) + [True])
        packed = A.pack(enc, train=False, decode="device")
        assert torch.equal(A.apply(packed, dev), A.apply(A.pack(enc, train=False), dev))
        for k, (name, data, e) in enumerate(raises):                  # every raising member, through `apply`
            with pytest.raises(type(e)) as got:
                A.apply(A.pack([good[0], data, good[1]], train=bool(k % 2), decode="device"), dev)
            assert str(got.value) == str(e), name
            if k % 8 == 0:
                with pytest.raises(type(e)) as got:
                    A.decode_images_device([good[0], data, good[1]], device=dev)
                assert str(got.value) == str(e), name


# ---- reproducibility --------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_batch_of_one_agree(dev, host_reference):
    el = JC.eligible()
    idx = list(range(0, len(el), 7)) + [len(el) - 3, len(el) - 1]
    enc = [el[i][5] for i in idx]
    a = A.decode_images_device(enc, device=dev, return_status=True)
    b = A.decode_images_device(enc, device=dev, return_status=True)
    assert torch.equal(a[0], b[0]) and not a[3].any() and not b[3].any()
    off = a[1].tolist()
    for k in (0, 5, len(enc) // 2, len(enc) - 1):
        one = A.decode_images_device([enc[k]], device=dev, return_status=True)
        assert torch.equal(one[0], a[0][off[k]:off[k + 1]]) and one[2].tolist() == [list(el[idx[k]][2:4])] and one[3].tolist() == [0]
