"""numpy restatements of the gradient norm of include/clibd_hip_optim.h, shared by tests/test_optim_cpu.py and tests/test_optim_gpu.py:
the norm in fp64, and the norm in fp32 summed in the kernel's documented order (so the error of that order is known without a GPU)."""
import numpy as np

CHUNK = 16384          # CLIBD_GRAD_NORM_CHUNK: 256 threads x 16 float4
THREADS = 256
NORM_FLOOR = 2.0 ** -22   # the fp32 result and its square root round by a few ulp
NORM_SIZES = [1, 63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 257 * CHUNK + 3]   # the last: a second partial on a pass-2 thread


def gradient(n: int, seed: int = 0) -> np.ndarray:
    """seeded normal values times a per-element scale spanning 2^-20 .. 2^20, fp32 [n]"""
    rng = np.random.default_rng(seed * 1000003 + n)
    return (rng.standard_normal(n) * np.exp2(rng.uniform(-20.0, 20.0, n))).astype(np.float32)


def norm_fp64(g: np.ndarray, grad_scale: float = 1.0) -> float:
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return float(grad_scale) * float(np.sqrt(np.sum(g * g)))


def _pairs(v: np.ndarray) -> np.ndarray:
    """neighbours added pairwise along the last axis until one value is left (fp32): wave_sum's order over 64 lanes"""
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def partials_fp32(g: np.ndarray) -> np.ndarray:
    """pass 1: one fp32 partial per chunk of CHUNK floats.  Thread t of a chunk takes float4 number k * 256 + t, k = 0 .. 15, and adds x^2,
    y^2, z^2, w^2 in turn with one rounding each (an fma: the square is exact in fp64, the sum rounds to fp32); 64 lanes pairwise; the four
    wave totals in order."""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    chunks = max(1, -(-g.size // CHUNK))
    a = np.zeros(chunks * CHUNK, dtype=np.float32)
    a[: g.size] = g
    a = a.reshape(chunks, CHUNK // (THREADS * 4), THREADS, 4).astype(np.float64)
    acc = np.zeros((chunks, THREADS), dtype=np.float32)
    for k in range(a.shape[1]):
        for e in range(4):
            acc = (acc.astype(np.float64) + a[:, k, :, e] * a[:, k, :, e]).astype(np.float32)
    waves = _pairs(acc.reshape(chunks, THREADS // 64, 64))
    return (((waves[:, 0] + waves[:, 1]).astype(np.float32) + waves[:, 2]).astype(np.float32) + waves[:, 3]).astype(np.float32)


def norm_fp32_kernel_order(g: np.ndarray, grad_scale: float = 1.0) -> np.float32:
    """pass 2 over `partials_fp32`: thread j adds partials j, j + 256, ... in fp64, an LDS tree (stride 128, 64, ... 1) adds the 256 sums;
    (float)(grad_scale * sqrt(sum))"""
    p = partials_fp32(g).astype(np.float64)
    part = np.zeros(THREADS, dtype=np.float64)
    for j0 in range(0, p.size, THREADS):          # thread j meets its partials in ascending order
        blk = p[j0 : j0 + THREADS]
        part[: blk.size] += blk
    d = THREADS // 2
    while d > 0:
        part[:d] = part[:d] + part[d : 2 * d]
        d //= 2
    return np.float32(np.float64(np.float32(grad_scale)) * np.sqrt(part[0]))


def norm_gate(g: np.ndarray, grad_scale: float = 1.0):
    """(fp64 norm, relative-error gate): 3 x the error of the fp32 restatement against fp64, at least NORM_FLOOR"""
    ref = norm_fp64(g, grad_scale)
    err32 = abs(float(norm_fp32_kernel_order(g, grad_scale)) - ref) / ref if ref > 0 else 0.0
    return ref, max(3.0 * err32, NORM_FLOOR), err32


def clip_coef(total_norm: np.float32, max_norm) -> np.float32:
    """torch's clip coefficient in fp32: min(1, max_norm / (total_norm + 1e-6)); no max_norm: 1"""
    if max_norm is None:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))
    return c if (np.isnan(c) or c < 1.0) else np.float32(1.0)
