"""numpy restatements of the gradient norm with a device divisor (include/clibd_hip_accum.h), in the style of tests/optim_reference.py
and built on it: the record in fp64, and the norm in fp32 summed in the kernel's documented order, so the gate of
tests/test_optim_gpu.py::test_norm_against_fp64 — 3 x the error of the fp32 restatement against fp64, at least 2^-22 — carries over with
the same formula.  Shared by tests/test_accum_cpu.py and tests/test_accum_gpu.py."""
import numpy as np

import optim_reference as OR

SIZES = [1, 3, OR.CHUNK, OR.CHUNK + 1, 3 * OR.CHUNK + 5]
DIVISORS = [None, 1.0, 7.0, float(2 ** 20 + 3), 0.0]      # None: a NULL pointer


def divisor_of(x) -> np.float32:
    """d = max(*divisor, 1) in fp32, the rule of clibd_mlm_ce_bf16's n_valid; NULL, 0, a negative value and NaN give 1"""
    if x is None:
        return np.float32(1.0)
    x = np.float32(x)
    return x if x > np.float32(1.0) else np.float32(1.0)


def norm_div_fp64(g: np.ndarray, grad_scale: float, divisor) -> float:
    return OR.norm_fp64(g, grad_scale) / float(divisor_of(divisor))


def norm_div_fp32_kernel_order(g: np.ndarray, grad_scale: float, divisor) -> np.float32:
    """optim_reference.norm_fp32_kernel_order's passes, then (float)(grad_scale * sqrt(sum) / d) with the product and quotient in fp64"""
    p = OR.partials_fp32(g).astype(np.float64)
    part = np.zeros(OR.THREADS, dtype=np.float64)
    for j0 in range(0, p.size, OR.THREADS):
        blk = p[j0 : j0 + OR.THREADS]
        part[: blk.size] += blk
    d = OR.THREADS // 2
    while d > 0:
        part[:d] = part[:d] + part[d : 2 * d]
        d //= 2
    return np.float32(np.float64(np.float32(grad_scale)) * np.sqrt(part[0]) / np.float64(divisor_of(divisor)))


def norm_div_gate(g: np.ndarray, grad_scale: float, divisor):
    """(fp64 norm / d, relative-error gate, the fp32 restatement's error): optim_reference.norm_gate's rule on the divided norm"""
    ref = norm_div_fp64(g, grad_scale, divisor)
    err32 = abs(float(norm_div_fp32_kernel_order(g, grad_scale, divisor)) - ref) / ref if ref > 0 else 0.0
    return ref, max(3.0 * err32, OR.NORM_FLOOR), err32


def coef_div(total_norm: np.float32, max_norm, divisor) -> np.float32:
    """clip(total_norm) / d in fp32: what the grouped update multiplies grad_scale by"""
    with np.errstate(all="ignore"):
        return np.float32(OR.clip_coef(total_norm, max_norm) / divisor_of(divisor))
