"""CPU checks of the device JPEG decode: the eleventh header (include/clibd_hip_jpeg.h) and its binding table, the host planner
(clibd_jpeg_plan) over the corpus of tests/jpeg_corpus.py and over cut and lying headers, host-side validation of clibd_jpeg_decode_u8,
the unit's register report, `collate_encoded(decode="device")` without a GPU, and csrc/jpeg_core.h — the planner and the scan decode
with their one bounded fetch — as a stand-alone host program under AddressSanitizer and UBSan over the corpus and its damage set."""
import ctypes
import io
import re
import struct
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import jpeg_corpus as JC  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_jpeg.h"
SYMBOLS = ["clibd_jpeg_decode_u8", "clibd_jpeg_plan", "clibd_jpeg_workspace_bytes"]
NOT_JPEG, TRUNCATED, SOF_KIND, COMPONENTS, DHT = 1, 2, 3, 5, 9


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


def _plan(data):
    from clibd_amd import augment as A

    return A.plan_streams([data], threads=1)[0]


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------
def test_jpeg_header_symbols_opening_comment_build_unit_and_plan_bytes():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening
    assert "jpeg" in build.SOURCES and build.SOURCES[-2:] == ["mlm", "rollout"] and HEADER in build._deps()
    assert build.CSRC / "jpeg_core.h" in build._deps()
    from clibd_amd import augment as A

    assert A.PLAN_BYTES == 4096 == int(re.search(r"#define CLIBD_JPEG_PLAN_BYTES (\d+)", HEADER.read_text()).group(1))


def test_reconstruction_kernels_use_no_scratch():
    """the compiler's resource remark for csrc/jpeg.hip: the IDCT (64 + 64 ints per lane) and the colour kernel keep their working set in
    registers; the Huffman kernel, divergent and latency-bound, is reported and not gated"""
    from clibd_amd import build

    rows = build.report_lines(build.resource_usage("jpeg"))
    print("\n".join(rows))
    assert len(rows) == 3 and sum("jpeg_entropy_kernel" in x for x in rows) == 1
    for kernel in ("jpeg_idct_kernel", "jpeg_colour_kernel"):
        row = [x for x in rows if kernel in x]
        assert len(row) == 1 and re.search(r"scratch=\s*0\b", row[0]) and re.search(r"lds=0\b", row[0]), row


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def test_plan_over_the_corpus():
    from clibd_amd import augment as A

    el = JC.eligible()
    plans = A.plan_streams([e[5] for e in el], threads=4)
    assert plans.dtype.itemsize == 4096 and len(plans) == len(el) >= 500
    for e, p in zip(el, plans):
        name, _, H, W, sub, data = e
        hs, vs = ((1, 1), (2, 1), (2, 2))[sub]
        assert (p["reason"], p["H"], p["W"], p["sampling"]) == (0, H, W, sub), name
        assert (p["mcus_x"], p["mcus_y"]) == (-(-W // (8 * hs)), -(-H // (8 * vs))), name
        assert p["blocks"] == p["mcus_x"] * p["mcus_y"] * (hs * vs + 2) and p["stream_len"] == len(data), name
        assert p["scan_begin"] == JC.scan_start(data), name
        assert (p["restart_interval"] > 0) == ("rst_" in name), name
    assert {e[1] for e in el} == {f"{s}-{o}" for s in ("444", "422", "420") for o in JC.OPTIONS}
    ne = JC.not_eligible()
    want = {"progressive": SOF_KIND, "png": NOT_JPEG, "gray": COMPONENTS, "cmyk": COMPONENTS}
    for name, data in ne.items():
        assert _plan(data)["reason"] == want[name], name
    assert _plan(b"")["reason"] == NOT_JPEG and _plan(b"\xff")["reason"] == NOT_JPEG and _plan(b"\xff\xd8")["reason"] == TRUNCATED
    bad = [d for d in JC.damaged() if d[1] == "bad_dht"]
    assert len(bad) == 1 and _plan(bad[0][2])["reason"] == DHT


def test_plan_refuses_what_libjpeg_would_not_read_as_ycbcr():
    a = JC.pixels(16, 16, "smooth", 0)
    rgb_ids = bytearray(JC.encode(a, quality=75, subsampling=0))
    sof = rgb_ids.index(b"\xff\xc0")
    sos = rgb_ids.index(b"\xff\xda")
    for k, cid in enumerate(b"RGB"):
        rgb_ids[sof + 10 + 3 * k] = cid
        rgb_ids[sos + 5 + 2 * k] = cid
    assert _plan(bytes(rgb_ids))["reason"] == 0                      # a JFIF APP0 settles it, whatever the ids (libjpeg's rule)
    app0 = rgb_ids.index(b"\xff\xe0")
    L = struct.unpack(">H", rgb_ids[app0 + 2:app0 + 4])[0]
    no_jfif = bytes(rgb_ids[:app0] + rgb_ids[app0 + 2 + L:])
    assert _plan(no_jfif)["reason"] == 7
    assert np.asarray(Image.open(io.BytesIO(no_jfif))).shape == (16, 16, 3)
    sampling = bytearray(JC.encode(a, quality=75, subsampling=0))
    sampling[sampling.index(b"\xff\xc0") + 11] = 0x12                # luma (1, 2)
    assert _plan(bytes(sampling))["reason"] == 6
    q16 = bytearray(JC.encode(a, quality=75, subsampling=0))
    q16[q16.index(b"\xff\xdb") + 4] |= 0x10                          # a DQT that claims 16-bit entries
    assert _plan(bytes(q16))["reason"] == 8
    p12 = bytearray(JC.encode(a, quality=75, subsampling=0))
    p12[p12.index(b"\xff\xc0") + 4] = 12
    assert _plan(bytes(p12))["reason"] == 4


def test_plan_survives_cut_and_lying_headers():
    name, _, H, W, sub, data = [e for e in JC.eligible() if e[0] == "33x47-smooth-420-q75-rst_blocks"][0]
    s = JC.scan_start(data)
    for cut in range(s):                                             # every proper prefix of the header
        assert _plan(data[:cut])["reason"] in (NOT_JPEG, TRUNCATED), cut
    assert _plan(data[:s])["reason"] == 0                            # the header alone plans; the scan's end is the device's business
    i, segments = 2, []
    while i < s:
        segments.append(i)
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    assert len(segments) >= 8
    for at in segments:
        for lie in (0, 1, 0xFFFF, len(data)):
            d = bytearray(data)
            d[at + 2:at + 4] = struct.pack(">H", lie & 0xFFFF)
            assert _plan(bytes(d))["reason"] != 0, (at, lie)
        true = data[at + 2] << 8 | data[at + 3]
        for lie in (true - 1, true + 1):                             # off by one: never a crash, never a read past the buffer
            d = bytearray(data)
            d[at + 2:at + 4] = struct.pack(">H", lie)
            _plan(bytes(d))


# ---- host validation ------------------------------------------------------------------------------------------------------------------
def test_decode_host_validation_needs_no_gpu(lib):
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    assert L.clibd_jpeg_workspace_bytes(0) == 0 and L.clibd_jpeg_workspace_bytes(-5) == 0
    assert L.clibd_jpeg_workspace_bytes(1) == 512 and L.clibd_jpeg_workspace_bytes(2112) == 2112 * 192
    assert L.clibd_jpeg_plan(None, 0, None) == -1 and b"null" in L.clibd_last_error()
    a, pl, out, off, st, ws = P(1 << 12), P(1 << 16), P(1 << 20), P(1 << 22), P(1 << 23), P(1 << 24)

    def dec(streams=a, nbytes=100, plans=pl, B=2, out=out, out_bytes=1000, offsets=off, status=st, w=ws, wbytes=192 * 64, blocks=64, phases=3):
        return L.clibd_jpeg_decode_u8(streams, nbytes, plans, B, out, out_bytes, offsets, status, w, wbytes, blocks, phases, None)

    for kw, word in ((dict(streams=None), b"null"), (dict(plans=None), b"null"), (dict(out=None), b"null"), (dict(offsets=None), b"null"),
                     (dict(status=None), b"null"), (dict(w=None), b"null"), (dict(B=0), b"non-positive batch"), (dict(B=-3), b"non-positive batch"),
                     (dict(B=65536), b"above 65535"), (dict(nbytes=0), b"non-positive size"), (dict(out_bytes=0), b"non-positive size"),
                     (dict(blocks=0), b"non-positive size"), (dict(phases=0), b"phases"), (dict(phases=4), b"phases"),
                     (dict(wbytes=192 * 64 - 1), b"clibd_jpeg_workspace_bytes"), (dict(w=P((1 << 24) + 8)), b"misaligned"),
                     (dict(plans=P((1 << 16) + 8)), b"misaligned pointer"), (dict(offsets=P((1 << 22) + 4)), b"misaligned pointer"),
                     (dict(status=P((1 << 23) + 2)), b"misaligned pointer")):
        assert dec(**kw) == -1, kw
        assert word in L.clibd_last_error() and b"jpeg_decode_u8" in L.clibd_last_error(), (kw, L.clibd_last_error())


# ---- the Python layer without a GPU -----------------------------------------------------------------------------------------------------
def _samples(encoded):
    return [(f"p{i}", e, torch.arange(5) + i, torch.zeros(20, dtype=torch.long), torch.zeros(20, dtype=torch.long), torch.ones(20, dtype=torch.long), i)
            for i, e in enumerate(encoded)]


def test_collate_encoded_device_form_without_a_gpu():
    from clibd_amd import augment as A
    from clibd_amd import simclr_views as V

    ne = JC.not_eligible()
    el = [e for e in JC.eligible() if e[2:4] == (33, 47) and "-q75-" in e[0]][:6]
    encoded = [el[0][5], ne["png"], el[1][5], el[2][5], ne["progressive"], el[3][5]]
    for train in (True, False):
        host = A.collate_encoded(_samples(encoded), train, torch.Generator().manual_seed(3), threads=2)
        devb = A.collate_encoded(_samples(encoded), train, torch.Generator().manual_seed(3), threads=2, decode="device")
        image = devb[1]
        assert sorted(image) == ["host_pixels", "jpeg", "offsets", "plans", "xforms"] and A.is_packed(image) and A.is_device_packed(image)
        assert not A.is_device_packed(host[1]) and A.is_packed(host[1])
        assert all(torch.is_tensor(v) and not v.is_cuda for v in image.values())
        assert torch.equal(image["xforms"], host[1]["xforms"]) and torch.equal(image["offsets"], host[1]["offsets"])
        assert host[0] == devb[0] and torch.equal(host[2], devb[2]) and torch.equal(host[6], devb[6])
        plans = image["plans"].numpy().view(A._PLAN).reshape(-1)
        assert plans["reason"].tolist() == [0, NOT_JPEG, 0, 0, SOF_KIND, 0]
        lens = [len(encoded[i]) for i in (0, 2, 3, 5)]
        assert image["jpeg"].numel() == sum(lens) and plans["stream_begin"][[0, 2, 3, 5]].tolist() == np.cumsum([0] + lens[:-1]).tolist()
        assert bytes(image["jpeg"].numpy()[lens[0]:lens[0] + lens[1]]) == encoded[2]
        assert plans["coef_begin"].tolist() == np.cumsum([0] + [int(b) if r == 0 else 0 for b, r in zip(plans["blocks"], plans["reason"])])[:6].tolist()
        off = image["offsets"].tolist()
        want = torch.cat([host[1]["data"][off[i]:off[i + 1]] for i in (1, 4)])
        assert torch.equal(image["host_pixels"], want)
    two_h = V.collate_two_views(encoded, torch.Generator().manual_seed(4))
    two_d = V.collate_two_views(encoded, torch.Generator().manual_seed(4), decode="device")
    assert V.is_packed(two_d) and torch.equal(two_h["xforms"], two_d["xforms"]) and "jpeg" in two_d and "data" not in two_d
    with pytest.raises(ValueError, match="decode must be one of"):
        A.collate_encoded(_samples(encoded), True, decode="gpu")
    for bad in ("gray", "cmyk"):                                     # today's error, today's message
        with pytest.raises(ValueError, match="image \\(the model takes RGB\\)"):
            A.collate_encoded(_samples([encoded[0], ne[bad]]), False, decode="device")
    # the default is the host path, unchanged
    assert sorted(A.collate_encoded(_samples(encoded), False)[1]) == ["data", "offsets", "xforms"]


# ---- jpeg_core.h as a stand-alone program under the sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return JC.build_program(tmp_path_factory.mktemp("jpeg_core"))


def _run(program, tmp_path, items, dump=False):
    return JC.run_program(program, tmp_path, items, dump)


def test_core_decodes_the_corpus_under_the_sanitizers(program, tmp_path):
    """every eligible stream ends with status 0, and libjpeg's reconstruction restated in numpy (tests/jpeg_corpus.py) turns the
    coefficients into PIL's pixels: the scan decode and the arithmetic the kernels implement, checked without a GPU"""
    el = JC.eligible()
    got = _run(program, tmp_path, [(e[0], e[5]) for e in el], dump=True)
    assert got == [(0, 0)] * len(el)
    for e, (status, coef) in zip(el, JC.read_dump(tmp_path / "dump", len(el))):
        assert status == 0 and np.array_equal(JC.reconstruct(coef, e[2], e[3], e[4]), np.asarray(Image.open(io.BytesIO(e[5])))), e[0]


def test_core_ends_clean_on_the_damage_set(program, tmp_path):
    dm = JC.damaged()
    kinds = {d[1] for d in dm}
    assert kinds == {"truncated", "flipped", "rst_removed", "rst_duplicated", "no_eoi", "bad_dht"}
    assert sum(d[1] == "truncated" for d in dm) == 36 and sum(d[1] == "flipped" for d in dm) == 16 * 12
    got = _run(program, tmp_path, [(d[0], d[2]) for d in dm] + list(JC.not_eligible().items()))
    for (name, kind, _), (reason, status) in zip(dm, got):
        if kind in ("truncated", "no_eoi", "rst_removed", "rst_duplicated"):
            assert reason == 0 and status >= 32, (name, reason, status)          # every truncation is reported
        elif kind == "bad_dht":
            assert (reason, status) == (DHT, -1), name
        else:
            assert reason != 0 or status == 0 or status >= 32, name
    assert [g for g in got[len(dm):]] == [(SOF_KIND, -1), (NOT_JPEG, -1), (COMPONENTS, -1), (COMPONENTS, -1)]


def test_core_reports_the_range_in_the_scan_and_leaves_the_rest_to_the_idct(program, tmp_path):
    r = JC.out_of_range()
    got = _run(program, tmp_path, list(r.items()), dump=True)
    assert got == [(0, 0), (0, 37)]                                  # `idct`: the scan is fine; `entropy`: the products leave int16
    status, coef = JC.read_dump(tmp_path / "dump", 2)[0]
    assert 16383 < np.abs(coef).max() <= 32767
