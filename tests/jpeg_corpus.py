"""The JPEG corpus of tests/test_jpeg_cpu.py and tests/test_jpeg_gpu.py, encoded with PIL from seeded arrays when a test asks for it
(nothing binary is committed), its deterministic damage set, the bundle format of tests/jpeg_fetch_main.cpp, and a numpy restatement of
libjpeg's default reconstruction (islow IDCT, fancy upsampling, fixed-point YCbCr -> RGB) from dequantised coefficients."""
import functools
import io
import os
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
from PIL import Image

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (33, 47), (64, 48)]
BIG = (256, 341)
CONTENTS = ("smooth", "noise")
SUBSAMPLING = (0, 1, 2)                      # 4:4:4, 4:2:2, 4:2:0
QUALITIES = (5, 75, 100)
OPTIONS = {"plain": {}, "optimize": {"optimize": True}, "rst_blocks": {"restart_marker_blocks": 3}, "rst_rows": {"restart_marker_rows": 1}}
SAMPLING_NAME = {0: "444", 1: "422", 2: "420"}


def pixels(H, W, content, seed):
    rng = np.random.default_rng(zlib.crc32(f"{H}x{W}/{content}/{seed}".encode()))
    noise = rng.integers(0, 256, size=(H, W, 3))
    if content == "noise":
        return noise.astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0), 255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1)], axis=-1)
    return np.clip(base + (noise - 128) * 0.15, 0, 255).astype(np.uint8)


def encode(a, fmt="JPEG", mode=None, **kw):
    im = Image.fromarray(a)
    if mode:
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, fmt, **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def eligible():
    """[(name, class name, H, W, subsampling, bytes)]: the full product over the small sizes, and one 256 x 341 per sampling."""
    out = []
    for (H, W) in SIZES:
        for content in CONTENTS:
            for sub in SUBSAMPLING:
                for q in QUALITIES:
                    for opt, kw in OPTIONS.items():
                        data = encode(pixels(H, W, content, q), quality=q, subsampling=sub, **kw)
                        out.append((f"{H}x{W}-{content}-{SAMPLING_NAME[sub]}-q{q}-{opt}", f"{SAMPLING_NAME[sub]}-{opt}", H, W, sub, data))
    for sub, opt in ((2, "plain"), (1, "rst_rows"), (0, "optimize")):
        data = encode(pixels(*BIG, "smooth", 90), quality=90 if sub == 2 else 75, subsampling=sub, **OPTIONS[opt])
        out.append((f"{BIG[0]}x{BIG[1]}-smooth-{SAMPLING_NAME[sub]}-{opt}", f"{SAMPLING_NAME[sub]}-{opt}", BIG[0], BIG[1], sub, data))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def not_eligible():
    """{name: bytes}: members the plan must leave to the host path"""
    a = pixels(33, 47, "smooth", 1)
    return {"progressive": encode(a, quality=75, progressive=True), "png": encode(a, fmt="PNG"),
            "gray": encode(a, mode="L", quality=75), "cmyk": encode(a, mode="CMYK", quality=75)}


# ---- the damage set -------------------------------------------------------------------------------------------------------------------
def scan_start(data):
    """index of the first entropy-coded byte: after the SOS header"""
    i = 2
    while True:
        assert data[i] == 0xFF
        m = data[i + 1]
        L = data[i + 2] << 8 | data[i + 3]
        i += 2 + L
        if m == 0xDA:
            return i


def restart_positions(data):
    s = scan_start(data)
    return [i for i in range(s, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def oversubscribe(data):
    """the first DHT's count of 1-bit codes set to 3: more codes than one bit can tell apart (the symbol list is lengthened to match)"""
    i = 2
    while True:
        m, L = data[i + 1], data[i + 2] << 8 | data[i + 3]
        if m == 0xC4:
            d = bytearray(data)
            add = 3 - d[i + 5]
            d[i + 5] = 3
            d[i + 2:i + 4] = struct.pack(">H", L + add)
            return bytes(d[:i + 21]) + bytes(add) + bytes(d[i + 21:])
        i += 2 + L


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, kind, bytes)], kind in truncated / flipped / rst_removed / rst_duplicated / no_eoi / bad_dht; seeded, the same every run"""
    out = []
    members = [e for e in eligible() if e[2:4] == (33, 47) and "-smooth-" in e[0] and "-q75-" in e[0]]
    for name, cls, H, W, sub, data in members:
        s = scan_start(data)
        n = len(data) - s
        for num in (1, 2, 3):
            out.append((f"{name}/trunc{num}of4", "truncated", data[:s + n * num // 4]))
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        for k, p in enumerate(sorted(rng.choice(np.arange(s, len(data) - 2), size=16, replace=False).tolist())):
            d = bytearray(data)
            d[p] ^= 1 << int(rng.integers(0, 8))
            out.append((f"{name}/flip{k}", "flipped", bytes(d)))
        out.append((f"{name}/no_eoi", "no_eoi", data[:-2]))
        rst = restart_positions(data)
        if rst:
            p = rst[len(rst) // 2]
            out.append((f"{name}/rst_removed", "rst_removed", data[:p] + data[p + 2:]))
            out.append((f"{name}/rst_duplicated", "rst_duplicated", data[:p + 2] + data[p:]))
    name, cls, H, W, sub, data = members[0]
    out.append((f"{name}/bad_dht", "bad_dht", oversubscribe(data)))
    return tuple(out)


def _patch_dqt(data, value):
    """every entry of every quantisation table set to `value`"""
    d, i = bytearray(data), 2
    while d[i + 1] != 0xDA:
        L = d[i + 2] << 8 | d[i + 3]
        if d[i + 1] == 0xDB:
            at = i + 4
            while at < i + 2 + L:
                d[at + 1:at + 65] = bytes([value]) * 64
                at += 65
        i += 2 + L
    return bytes(d)


@functools.lru_cache(maxsize=None)
def out_of_range():
    """{name: bytes}: valid syntax, values outside the range in which libjpeg's IDCT forms agree, so the device must hand the image to
    the host (CLIBD_JPEG_RANGE = 37) — from either place that can tell.  `idct`: a flat bright 16 x 16 image at q100 whose quantisers
    were then set to 20: every DC coefficient is about 20 x 976, inside int16 but above the 16383 the IDCT kernel accepts.  `entropy`: a
    noise image at q100 with the quantisers set to 255: the products leave int16 in the scan decode already."""
    flat = encode(np.full((16, 16, 3), 250, dtype=np.uint8), quality=100, subsampling=2)
    noise = encode(pixels(16, 16, "noise", 3), quality=100, subsampling=0)
    return {"idct": _patch_dqt(flat, 20), "entropy": _patch_dqt(noise, 255)}


# ---- jpeg_core.h as a host program -------------------------------------------------------------------------------------------------------
def build_program(directory):
    """tests/jpeg_fetch_main.cpp built as plain host C++ with -fsanitize=address,undefined; the runtimes are linked in statically, so the
    program needs nothing preloaded and does not mind what the environment preloads"""
    root = Path(__file__).resolve().parents[1]
    exe = Path(directory) / "jpeg_fetch_main"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", str(root / "tests" / "jpeg_fetch_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_program(exe, directory, items, dump=False):
    """[(reason, status)] per item; fails unless the program ends clean (exit 0, no sanitizer report)"""
    directory = Path(directory)
    write_bundle(directory / "bundle", items)
    cmd = [str(exe), str(directory / "bundle")] + ([str(directory / "dump")] if dump else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    assert [x[0] for x in rows] == [n for n, _ in items]
    return [(int(x[1]), int(x[2])) for x in rows]


def write_bundle(path, items):
    """items: [(name, bytes)] in the record format tests/jpeg_fetch_main.cpp reads"""
    with open(path, "wb") as f:
        for name, data in items:
            n = name.encode()
            f.write(struct.pack("<I", len(n)) + n + struct.pack("<I", len(data)) + data)


# ---- libjpeg's default reconstruction, restated -----------------------------------------------------------------------------------------
def _islow_1d(v, shift):
    """jidctint.c's 1-D pass over the last axis of an int64 array [..., 8]"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1) + r >> shift


def idct_islow(blocks):
    """int16 [n, 64] natural order -> uint8 [n, 8, 8]"""
    c = blocks.astype(np.int64).reshape(-1, 8, 8)
    ws = _islow_1d(c.transpose(0, 2, 1), 11).transpose(0, 2, 1)     # pass 1 runs down the columns
    return np.clip(_islow_1d(ws, 18) + 128, 0, 255).astype(np.uint8)


def _plane(samples, rows, cols):
    return samples.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)


def _upsample(c, sub, H, W):
    hs, vs = (1, 1) if sub == 0 else (2, 1) if sub == 1 else (2, 2)
    dw, dh = -(-W // hs), -(-H // vs)
    c = c[:dh, :dw].astype(np.int64)
    if sub == 0:
        return c
    if dw <= 2:                                                     # jinit_upsampler: replication for narrow components
        return np.repeat(np.repeat(c, vs, axis=0), hs, axis=1)
    if sub == 1:
        left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
        out = np.empty((dh, 2 * dw), dtype=np.int64)
        out[:, 0::2] = (3 * c + left + 1) >> 2
        out[:, 1::2] = (3 * c + right + 2) >> 2
        out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
        return out
    up, down = np.concatenate([c[:1], c[:-1]], 0), np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * dh, 2 * dw), dtype=np.int64)
    for v, other in ((0, up), (1, down)):
        cs = 3 * c + other
        left, right = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[v::2, 0::2] = (3 * cs + left + 8) >> 4
        out[v::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def reconstruct(coef, H, W, sub):
    """RGB uint8 [H, W, 3] from the dequantised coefficients int16 [blocks, 64] in the layout of jpeg_core.h (luma plane, Cb, Cr)"""
    hs, vs = (1, 1) if sub == 0 else (2, 1) if sub == 1 else (2, 2)
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    mcus = mx * my
    s = idct_islow(coef)
    Y = _plane(s[:mcus * hs * vs], my * vs, mx * hs)[:H, :W].astype(np.int64)
    cb = _upsample(_plane(s[mcus * hs * vs:mcus * (hs * vs + 1)], my, mx), sub, H, W)[:H, :W] - 128
    cr = _upsample(_plane(s[mcus * (hs * vs + 1):], my, mx), sub, H, W)[:H, :W] - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def read_dump(path, count):
    """[(status, coef int16 [blocks, 64])] of the dump file tests/jpeg_fetch_main.cpp writes"""
    raw = open(path, "rb").read()
    out, at = [], 0
    for _ in range(count):
        status, blocks = struct.unpack_from("<ii", raw, at)
        at += 8
        out.append((status, np.frombuffer(raw, dtype="<i2", count=blocks * 64, offset=at).reshape(blocks, 64)))
        at += blocks * 128
    assert at == len(raw)
    return out
