"""CPU-importable half of the bf16 GEMM form tests (tests/test_gemm_forms_gpu.py, tests/test_gemm_forms_cpu.py).

Holds, for every bf16 GEMM entry point of clibd_amd/csrc/gemm.hip, gemm256.hip and gemm256_tn.hip:

* `Case`: one launch (shape, epilogue fields, strides, K hole, split) and `Draws`: its seeded operands, made once per shape;
* the Python mirror of the host routing (`epilogue_kind`, `takes_256`, `nt_splitk_takes`, `tn_splitk_takes`, `transpose_form`);
* `reference`: the operation in fp64 from the bf16 operands, together with `s`, the fp64 sum of magnitudes of everything that was
  added to make each element, carried through the epilogue like the value;
* `restate`: the same operation in fp32 torch with the kernels' rounding points (read from store_row16 / store_row8 / gemm256_body);
* `judge`: e = |got - ref| / max(|ref|, 2^-10 s) per element, the worst element and its place;
* the case lists both test modules walk.

Rounding points of the kernels, as restated here (gemm_common.h):
  v = fp32(acc + rank-8 term) + bias                 (the rank update is one more MFMA k-step into the same accumulator)
  dropout multiplies v by 0 or 1/(1-p)
  GELU_SAVE_GRAD[_U8|_E12] (all kernels, EPI_GELU_SAVE*, EPI_ROWNORM_GELU): x = bf16(v); y = gelu(x); g = gelu'(x);
        out_pre = bf16(g) | code(g) (code formed from the fp32 g) | e4m7(bf16(g));  v = y
  otherwise, with out_pre: out_pre = bf16(v) and v = bf16(v)  -> ACT_GELU with out_pre is gelu of the ROUNDED pre-activation,
  ACT_GELU without out_pre (generic and EPI_GELU): gelu of the fp32 value
  GELU_GRAD: v *= gelu'(aux);  MUL_AUX*: v *= aux (decoded);  ADD_AUX: v += aux;  then v += residual
  out_f32 = v;  out_bf16 = bf16(v): every bf16 output is rounded once, at its store.

How `s` passes through GELU: gelu is 1.13-Lipschitz and |gelu(x)| <= |x|, gelu' is 1-Lipschitz (|gelu''| <= 0.8), so an input whose
terms have magnitude sum s gives an output whose error scale is at most s: s passes through GELU and GELU' unchanged.  The
multiplying forms scale it by |aux| / |gelu'(aux)| / the drop factor, the adding forms add |aux| / |residual| to it."""
import math
import os
import re
from dataclasses import dataclass
from typing import Optional

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ACT_NONE, ACT_GELU, ACT_GELU_GRAD, ACT_GELU_SAVE_GRAD, ACT_MUL_AUX, ACT_ADD_AUX, ACT_GELU_SAVE_GRAD_U8, ACT_MUL_AUX_U8 = range(8)
ACT_GELU_SAVE_GRAD_E12, ACT_MUL_AUX_E12 = 8, 9
SAVE_ACTS = (ACT_GELU_SAVE_GRAD, ACT_GELU_SAVE_GRAD_U8, ACT_GELU_SAVE_GRAD_E12)
ACT_NAMES = ("none", "gelu", "gelu_grad", "gelu_save", "mul_aux", "add_aux", "gelu_save_u8", "mul_aux_u8", "gelu_save_e12", "mul_aux_e12")

# common.h: the one-byte gelu' code
GELUQ_LO = -0.1328125
GELUQ_STEP = float(torch.tensor(1.265625 / 255.0, dtype=F32))
GELUQ_INV = float(torch.tensor(255.0 / 1.265625, dtype=F32))

# routing constants (test_gemm_forms_cpu.py checks each against the sources)
T_M, T_N, T_K = 256, 256, 64           # gemm256.hip
BM, BN, BK = 128, 128, 64              # gemm.hip
MIN_M_256, MIN_TILES_256 = 1024, 128   # gemm256_try_launch
WS_GROUP = 6                           # CLIBD_WS_GROUP: column tiles per W-stationary group
(EPI_GENERIC, EPI_BF16, EPI_GELU_SAVE, EPI_MUL_AUX, EPI_RES_F32, EPI_RES_F32_DROP, EPI_SPLITK_F32, EPI_ADD_AUX, EPI_GELU_SAVE_U8, EPI_MUL_AUX_U8,
 EPI_RES_F32_COPY, EPI_ROWNORM_GELU, EPI_GELU_SAVE_12, EPI_MUL_AUX_12, EPI_GELU, EPI_F32) = range(16)
EPI_NAMES = ("GENERIC", "BF16", "GELU_SAVE", "MUL_AUX", "RES_F32", "RES_F32_DROP", "SPLITK_F32", "ADD_AUX", "GELU_SAVE_U8", "MUL_AUX_U8",
             "RES_F32_COPY", "ROWNORM_GELU", "GELU_SAVE_12", "MUL_AUX_12", "GELU", "F32")
LN_EPS = 1e-6

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    act: int = ACT_NONE
    bias: bool = False
    rank: bool = False
    residual: bool = False
    out_pre: bool = False
    out_bf16: bool = False
    out_f32: bool = False
    drop: float = 0.0
    split_k: int = 1
    hole: Optional[tuple] = None      # (k0, length) of clibd_gemm_bf16_nt_khole
    scale: float = 1.0                # multiplies W, v and the bias: pre-activations span about +-4 * scale
    strided: bool = False
    rank_scale: float = 1.0           # multiplies u (0.1: an adapter-sized update)
    fold: Optional[str] = None        # "producer" (row_sums) | "consumer" (row_stats + col_sum_w)
    seed: int = 0
    unfolded: bool = False            # fold == "consumer": judge against the un-folded LayerNorm -> Linear -> GELU (else the folded formula in fp64)
    draw_M: int = 0                   # > M: the operands are the first M rows of the draws of an M = draw_M case (threshold pairs)

    @property
    def aux(self):
        return {ACT_GELU_GRAD: "bf16", ACT_MUL_AUX: "bf16", ACT_ADD_AUX: "bf16", ACT_MUL_AUX_U8: "u8", ACT_MUL_AUX_E12: "e12"}.get(self.act)

    @property
    def has_pre(self):
        return self.out_pre or self.act in SAVE_ACTS

    @property
    def id(self):
        p = [f"{self.M}x{self.N}x{self.K}", ACT_NAMES[self.act]]
        p += [n for n, on in (("bias", self.bias), ("rank", self.rank), ("res", self.residual), ("pre", self.out_pre), ("obf", self.out_bf16),
                              ("of32", self.out_f32), ("strided", self.strided)) if on]
        if self.drop > 0:
            p.append(f"drop{self.drop}")
        if self.split_k > 1:
            p.append(f"split{self.split_k}")
        if self.hole:
            p.append(f"hole{self.hole[0]}+{self.hole[1]}")
        if self.scale != 1.0:
            p.append(f"x{self.scale}")
        if self.fold:
            p.append(self.fold + ("_unfolded" if self.unfolded else ""))
        return "-".join(p)


def epilogue_kind(c: Case) -> int:
    """gemm_common.h epilogue_kind()"""
    if c.split_k > 1:
        return EPI_GENERIC
    drop, pre, res, f32, b16, aux = c.drop > 0, c.has_pre, c.residual, c.out_f32, c.out_bf16, c.aux is not None
    if c.fold == "producer":
        return EPI_RES_F32_COPY if (c.act == ACT_NONE and not drop and not pre and res and f32 and b16 and not c.rank and c.bias) else -1
    if c.fold == "consumer":
        return EPI_ROWNORM_GELU if (c.act == ACT_GELU_SAVE_GRAD and not drop and pre and not res and not f32 and b16 and not c.rank and c.bias) else -1
    plain_bf16 = not drop and not res and not f32 and b16
    if c.act == ACT_NONE and plain_bf16 and not pre:
        return EPI_BF16
    if c.act == ACT_GELU_SAVE_GRAD and plain_bf16 and pre:
        return EPI_GELU_SAVE
    if c.act == ACT_GELU and plain_bf16 and not pre:
        return EPI_GELU
    if c.act == ACT_MUL_AUX and plain_bf16 and not pre and aux:
        return EPI_MUL_AUX
    if c.act == ACT_ADD_AUX and plain_bf16 and not pre and aux:
        return EPI_ADD_AUX
    if c.act == ACT_GELU_SAVE_GRAD_U8 and plain_bf16 and pre:
        return EPI_GELU_SAVE_U8
    if c.act == ACT_MUL_AUX_U8 and plain_bf16 and not pre and aux:
        return EPI_MUL_AUX_U8
    if c.act == ACT_GELU_SAVE_GRAD_E12 and plain_bf16 and pre:
        return EPI_GELU_SAVE_12
    if c.act == ACT_MUL_AUX_E12 and plain_bf16 and not pre and aux:
        return EPI_MUL_AUX_12
    if c.act in (ACT_GELU_SAVE_GRAD_E12, ACT_MUL_AUX_E12):
        return -1
    if c.act == ACT_NONE and not pre and res and f32 and not b16:
        return EPI_RES_F32_DROP if drop else EPI_RES_F32
    if c.act == ACT_NONE and not drop and not pre and not res and f32 and not b16:
        return EPI_F32
    return EPI_GENERIC


def takes_256(c: Case) -> bool:
    """gemm_impl + gemm256_try_launch: does this launch run the 256x256 kernel?  (operands here are far below 2^32 bytes)"""
    nk = c.K // T_K
    if c.hole is not None and c.hole[1] > 0:
        return False
    if c.K % T_K or nk < 4 or nk & 1 or c.N % T_N or c.split_k > 1:
        return False
    tiles = -(-c.M // T_M) * (c.N // T_N)
    if c.M < MIN_M_256 or tiles < MIN_TILES_256:
        return False
    return epilogue_kind(c) >= 0


def nt_splitk_takes(M, N, K) -> bool:
    """gemm256_splitk_launch (ops.gemm_nt_splitk tests the same conditions before it calls)"""
    nk = K // T_K
    return K % T_K == 0 and nk >= 8 and nk % 2 == 0 and N % T_N == 0 and M >= 1


def tn_splitk_takes(M, Na, Nb) -> bool:
    """gemm256_tn_splitk_launch / tn_splitk_impl"""
    return M > 0 and M % 128 == 0 and M // 64 >= 4 and Na % 256 == 0 and Nb % 256 == 0


def plan_k_slices(nk, tiles, cus):
    """gemm_common.h plan_k_slices -> (splits, K-tiles per slice)"""
    splits = max(1, cus // max(tiles, 1))
    splits = max(1, min(splits, nk // 4))
    nks = -(-nk // splits)
    nks += nks & 1
    nks = min(max(nks, 4), nk)
    splits = -(-nk // nks)
    while nk - (splits - 1) * nks < 4 and nks < nk:
        nks = min(nks + 2, nk)
        splits = -(-nk // nks)
    return splits, nks


def transpose_form(C, ld_in, ld_out) -> str:
    """transpose_impl, for 16-byte aligned bases: 'general' | 'fast64' (ld_out < 1024) | 'fast256'"""
    if C % 8 or ld_in % 8 or ld_out % 8:
        return "general"
    return "fast256" if ld_out >= 1024 else "fast64"


def locate(c: Case, m: int, n: int) -> str:
    """tile and wave of output element (m, n), for the failure message"""
    if takes_256(c):   # gemm256_body: wave (wm, wn) owns rows 64 wn .. + 63 and columns 128 wm .. + 127 of the tile; a lane owns 8 columns
        return (f"256x256 tile (m-tile {m // T_M}, n-tile {n // T_N}), wave rows {m % T_M // 64 * 64}..+63, wave columns {n % T_N // 128 * 128}..+127 "
                f"(64-column slice {n % T_N // 64}), lane strip columns {n // 8 * 8}..+7")
    return (f"128x128 tile (m-tile {m // BM}, n-tile {n // BN}), wave rows {m % BM // 64 * 64}..+63, 64-column slice {n % BN // 64}, "
            f"lane strip columns {n // 16 * 16}..+15")


# ------------------------------------------------------------------------------------------------ operands
class Draws:
    """Seeded operands of one shape, made on the host on first use and cached per device.  Every tensor is its own draw with its own
    non-zero mean, so a swapped or transposed operand changes the result."""
    _TAGS = ("A", "W", "u", "v", "bias", "aux", "codes", "g12", "res", "prev", "x1", "gamma", "beta", "w1")

    def __init__(self, M, N, K, seed=0, scale=1.0, hole=None, rank_scale=1.0):
        self.M, self.N, self.K, self.seed, self.scale, self.hole, self.rank_scale = M, N, K, seed, scale, hole, rank_scale
        self._host, self._dev = {}, {}

    def _gen(self, tag):
        return torch.Generator().manual_seed(1000003 * self.seed + 7919 * self._TAGS.index(tag) + self.M * 31 + self.N * 17 + self.K)

    def host(self, tag):
        if tag in self._host:
            return self._host[tag]
        M, N, K, sc, g = self.M, self.N, self.K, self.scale, self._gen(tag)
        keff = K - (self.hole[1] if self.hole else 0)
        if tag == "A":
            t = (torch.randn(M, K, generator=g) + 0.05).to(BF16)
        elif tag == "W":
            t = (torch.randn(N, K, generator=g) * (1.3 * sc / math.sqrt(keff)) + 0.02 * sc / math.sqrt(keff)).to(BF16)
        elif tag == "u":
            t = ((torch.randn(M, 8, generator=g) * 0.5 + 0.1) * self.rank_scale).to(BF16)
        elif tag == "v":
            t = (torch.randn(N, 8, generator=g) * (0.3 * sc) - 0.05 * sc).to(BF16)
        elif tag == "bias":
            t = torch.randn(N, generator=g) * (0.3 * sc) + 0.1 * sc
        elif tag == "aux":      # a pre-activation (GELU_GRAD) or a factor / addend
            t = (torch.randn(M, N, generator=g) * 1.3 + 0.1).to(BF16)
        elif tag == "codes":    # one-byte gelu' codes: every value occurs
            t = torch.randint(0, 256, (M, N), generator=g, dtype=torch.uint8)
        elif tag == "g12":      # bf16 gelu' values over its whole range, a tenth of them in the flushed tail |g| < 2^-14
            v = torch.rand(M, N, generator=g) * 1.258 - 0.129
            tiny = torch.rand(M, N, generator=g) < 0.1
            t = torch.where(tiny, v * 2e-5, v).to(BF16)
        elif tag == "res":
            t = torch.randn(M, N, generator=g) * 1.5 + 0.2
        elif tag == "prev":     # what an accumulating output holds before the launch
            t = torch.randn(M, N, generator=g) * 2.0 - 0.3
        elif tag == "x1":       # LN-fold consumer: the fp32 residual stream the statistics come from
            t = torch.randn(M, K, generator=g) * 1.5 + 0.2
        elif tag == "gamma":
            t = 1.0 + 0.2 * torch.randn(K, generator=g)
        elif tag == "beta":
            t = 0.1 * torch.randn(K, generator=g)
        elif tag == "w1":
            t = torch.randn(N, K, generator=g) * (1.3 / math.sqrt(K)) + 0.02 / math.sqrt(K)
        else:
            raise KeyError(tag)
        self._host[tag] = t
        return t

    def get(self, tag, device):
        device = torch.device(device)
        if device.type == "cpu":
            return self.host(tag)
        key = (tag, str(device))
        if key not in self._dev:
            self._dev[key] = self.host(tag).to(device)
        return self._dev[key]


class _Rows:
    """the first M rows of a Draws made for more rows"""
    _ROW_TAGS = ("A", "u", "aux", "codes", "g12", "res", "prev", "x1")

    def __init__(self, d, M):
        self.d, self.M = d, M

    def get(self, tag, device):
        t = self.d.get(tag, device)
        return t[:self.M] if tag in self._ROW_TAGS else t


_current = {}


def draws_for(c: Case):
    """one live Draws at a time: the case lists are ordered by shape"""
    key = (max(c.M, c.draw_M), c.N, c.K, c.seed, c.scale, c.hole, c.rank_scale)
    if _current.get("key") != key:
        _current.clear()
        _current["key"] = key
        _current["draws"] = Draws(*key)
    d = _current["draws"]
    return d if d.M == c.M else _Rows(d, c.M)


# ------------------------------------------------------------------------------------------------ gelu, codes
def bfr(x):
    return x.to(BF16).to(x.dtype)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def kernel_gelu_and_grad(x):
    """common.h gelu_and_grad_x2 in fp32 torch: erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, absolute), exp(-x^2/2) as exp2(-(K|x|)^2)"""
    K = 0.84932180028801907
    P = 0.3275911 * 0.70710678118654752 / K
    ax = x.abs() * K
    t = 1.0 / (ax * P + 1.0)
    poly = ((((0.5307027145 * t - 0.7265760135) * t + 0.7107068705) * t - 0.142248368) * t + 0.127414796) * t
    e = torch.exp2(-(ax * ax))
    cdf = torch.copysign(0.5 - poly * e, x) + 0.5
    return x * cdf, (x * e) * 0.3989422804014327 + cdf


def kernel_gelu_grad(x):
    """common.h gelu_grad_f (fast_erf) in fp32 torch"""
    xs = x * 0.70710678118654752
    ax = xs.abs()
    t = 1.0 / (1.0 + 0.3275911 * ax)
    y = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    erf = torch.copysign(1.0 - y * torch.exp(-ax * ax), xs)
    return 0.5 * (1.0 + erf) + x * (0.3989422804014327 * torch.exp(-0.5 * x * x))


def u8_encode(g32):
    """geluq_pack4: code = sat_u8(rint(fma(g, INV, -LO INV)))"""
    return torch.clamp(torch.round(g32 * GELUQ_INV + (-GELUQ_LO * GELUQ_INV)), 0, 255).to(torch.uint8)


def u8_decode(codes, dtype=F32):
    """geluq_unpack4: fma(code, STEP, LO)"""
    return codes.to(dtype) * GELUQ_STEP + GELUQ_LO


def _bf16_bits(x_bf16):
    return x_bf16.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def e12_codes(x_bf16):
    """gelu12_code_bits of bf16 values -> int64 12-bit codes"""
    b = _bf16_bits(x_bf16)
    t = b & 0x7FFF
    u = torch.where(t >= (113 << 7), t - (112 << 7), torch.zeros_like(t)).clamp(max=0x7FF)
    return ((b >> 4) & 0x800) | u


def e12_value(codes):
    """gelu12_val: 12-bit codes -> fp32"""
    u = codes & 0x7FF
    t = torch.where(u > 0, u + (112 << 7), torch.zeros_like(u))
    bits = (((codes & 0x800) << 4) | t) << 16
    return bits.to(torch.int32).view(F32)


def e12_pack(x_bf16):
    """[M, N] bf16 -> uint8 [M, 3N/2]: eight columns = three little-endian dwords (gelu12_pack8)"""
    M, N = x_bf16.shape
    c = e12_codes(x_bf16).view(M, N // 8, 8)
    w0 = (c[..., 0] | (c[..., 1] << 12) | (c[..., 2] << 24)) & 0xFFFFFFFF
    w1 = ((c[..., 2] >> 8) | (c[..., 3] << 4) | (c[..., 4] << 16) | (c[..., 5] << 28)) & 0xFFFFFFFF
    w2 = ((c[..., 5] >> 4) | (c[..., 6] << 8) | (c[..., 7] << 20)) & 0xFFFFFFFF
    w = torch.stack([w0, w1, w2], dim=-1)
    by = torch.stack([(w >> (8 * i)) & 0xFF for i in range(4)], dim=-1)
    return by.to(torch.uint8).view(M, 3 * N // 2)


def e12_unpack(buf, N):
    """uint8 [M, 3N/2] -> fp32 [M, N] (gelu12_unpack8)"""
    M = buf.shape[0]
    b = buf.contiguous().view(M, N // 8, 12).to(torch.int64)
    w = [b[..., 4 * i] | (b[..., 4 * i + 1] << 8) | (b[..., 4 * i + 2] << 16) | (b[..., 4 * i + 3] << 24) for i in range(3)]
    c = [w[0] & 0xFFF, (w[0] >> 12) & 0xFFF, (w[0] >> 24) | ((w[1] & 0xF) << 8), (w[1] >> 4) & 0xFFF, (w[1] >> 16) & 0xFFF,
         (w[1] >> 28) | ((w[2] & 0xFF) << 4), (w[2] >> 8) & 0xFFF, w[2] >> 20]
    return e12_value(torch.stack(c, dim=-1).view(M, N))


def drop_factor64(seed, M, N, p, device):
    """oracle.clibd_oracle.drop_factor at element index m * N + n (ops.gemm_nt passes drop_ld = N), as fp64 on `device`"""
    from oracle.clibd_oracle import drop_factor

    idx = torch.arange(M * N, dtype=torch.int64, device=device).view(M, N)
    return drop_factor(seed, idx, p).to(device=device, dtype=F64)


def drop_site(c: Case):
    """(p, seed) of a case's dropout site"""
    return c.drop, (0x9E3779B1 * (c.seed + 1) + c.M) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the operation
def _kept(c: Case, t):
    """operand columns outside the K hole"""
    if not c.hole or c.hole[1] == 0:
        return t
    k0, ln = c.hole
    return torch.cat([t[:, :k0], t[:, k0 + ln:]], dim=1)


def _aux_value(c: Case, d: Draws, device, dt):
    if c.aux == "bf16":
        return d.get("aux", device).to(dt)
    if c.aux == "u8":
        return u8_decode(d.get("codes", device), dt)
    if c.aux == "e12":
        return e12_value(e12_codes(d.get("g12", device))).to(dt)
    return None


def _fold_consumer_inputs(d, device, unfolded, given=None):
    """LN-fold consumer.  unfolded: (x1b, w1, gamma, beta, b1) as fp64 for the un-folded statement; else the folded operands (x1b fp32, wg fp32,
    s_n, b', mean, rstd): `given` (what ops.ln_fold_weights / ops.rowsum_finalize made, on the GPU) or, on the CPU, as rowsum_finalize_kernel and
    ln_fold_weights_kernel make them."""
    x1, w1, gamma, beta, b1 = (d.get(k, device) for k in ("x1", "w1", "gamma", "beta", "bias"))
    x1b = x1.to(BF16)
    if unfolded:
        return x1b.double(), w1.double(), gamma.double(), beta.double(), b1.double()
    if given is not None:
        return (x1b.float(), given["wg"].float(), given["s_n"], given["bp"], given["stats"][:, 0], given["stats"][:, 1])
    H = x1.shape[1]
    t, q = x1.double().sum(-1), (x1 * x1).double().sum(-1)          # (per-slice fp32 sums in the product; merged in fp64 either way)
    mean_d = t / H
    var = ((q - mean_d * t) / H).float().clamp(min=0.0)
    wg = bfr(w1 * gamma)
    return x1b.float(), wg, wg.sum(-1), b1 + (w1 * beta).sum(-1), mean_d.float(), torch.rsqrt(var + LN_EPS)


def _run(c: Case, device, exact: bool, cache=None, given=None):
    """The operation of `c`: exact -> fp64 with no rounding, returns {output: (ref, s, class)}; else fp32 with the kernels' rounding
    points, returns {output: (value as fp32, None, class)}.  Byte-coded outputs are returned decoded."""
    d = draws_for(c)
    dt = F64 if exact else F32
    R = (lambda x: x) if exact else bfr
    M, N = c.M, c.N
    key = (c.M, c.draw_M, c.N, c.K, c.seed, c.scale, c.rank_scale, c.hole, c.bias, c.rank, c.fold == "consumer", c.unfolded, str(device), exact)
    if cache is not None and cache.get("key") == key:
        pre, s = cache["pre"], cache["s"]
    else:
        if c.fold == "consumer":
            if exact and c.unfolded:
                x, w1, gamma, beta, b1 = _fold_consumer_inputs(d, device, True)
                mu = x.mean(-1, keepdim=True)
                rstd = (x.var(-1, unbiased=False, keepdim=True) + LN_EPS).rsqrt()
                xn = (x - mu) * rstd * gamma + beta
                pre = xn @ w1.T + b1
                s = xn.abs() @ w1.abs().T + b1.abs()
            elif exact:   # the folded formula itself, in fp64, from the fp32 operands the kernel is given
                x, wg, s_n, bp, mean, rstd = (t.double() for t in _fold_consumer_inputs(d, device, False, given))
                pre = rstd[:, None] * (x @ wg.T - mean[:, None] * s_n[None, :]) + bp[None, :]
                s = rstd[:, None] * (x.abs() @ wg.abs().T + mean.abs()[:, None] * s_n.abs()[None, :]) + bp.abs()[None, :]
            else:
                x, wg, s_n, bp, mean, rstd = _fold_consumer_inputs(d, device, False, given)
                acc = x @ wg.T
                pre = torch.addcmul(bp[None, :], rstd[:, None], torch.addcmul(acc, -mean[:, None], s_n[None, :]))   # fold_rownorm8 (two roundings; fma: one each)
                s = None
        else:
            A, W = _kept(c, d.get("A", device)).to(dt), _kept(c, d.get("W", device)).to(dt)
            pre = A @ W.T
            s = A.abs() @ W.abs().T if exact else None
            if c.rank:
                u, v = d.get("u", device).to(dt), d.get("v", device).to(dt)
                pre = pre + u @ v.T
                if exact:
                    s = s + u.abs() @ v.abs().T
            if c.bias:
                b = d.get("bias", device).to(dt)
                pre = pre + b
                if exact:
                    s = s + b.abs()
        if cache is not None:
            cache.clear()
            cache.update(key=key, pre=pre, s=s)
    out = {}
    v = pre
    if c.split_k > 1:   # store_row16: atomic adds onto what the output holds
        prev = d.get("prev", device).to(dt)
        out["out_f32"] = (prev + v, (s + prev.abs()) if exact else None, "f32_acc")
        return out
    if c.drop > 0:
        p, seed = drop_site(c)
        f = drop_factor64(seed, M, N, p, device).to(dt)
        v = v * f
        if exact:
            s = s * f
    # outputs downstream of an intermediate bf16 rounding (x = bf16(v) of the GELU_SAVE forms, v = bf16(v) behind out_pre) are classes of their
    # own ("_mid"): the rounding is 2^-9 |x|, which the floor 2^-10 s does not cover, and it would otherwise set the bound of every bf16 / fp32 output
    # ("_gg": behind ACT_GELU_GRAD the A&S erf's ABSOLUTE error of 1.5e-7 in gelu'(aux) is multiplied by the accumulator: where gelu'(aux) and the residual
    #  are both nearly zero that is up to 2e-2 of the floor, five times the bf16 rounding that sets the plain classes)
    fold_cls = "_fold" if c.unfolded else "_mid" if c.has_pre else "_gg" if c.act == ACT_GELU_GRAD else ""
    dg_cls = "_fold" if c.unfolded else ""
    if c.act in SAVE_ACTS:
        x = R(v)
        y, g = (gelu(x), gelu_grad(x)) if exact else kernel_gelu_and_grad(x)
        if exact:
            cls = {ACT_GELU_SAVE_GRAD: "dg_bf16", ACT_GELU_SAVE_GRAD_U8: "dg_u8", ACT_GELU_SAVE_GRAD_E12: "dg_e12"}[c.act] + dg_cls
            out["out_pre"] = (g, s, cls)
            out["pre_act"] = (x, s, None)        # (for the derived one-byte bound; not an output)
        elif c.act == ACT_GELU_SAVE_GRAD:
            out["out_pre"] = (bfr(g), None, "dg_bf16" + dg_cls)
        elif c.act == ACT_GELU_SAVE_GRAD_U8:
            out["out_pre"] = (u8_decode(u8_encode(g)), None, "dg_u8")
        else:
            out["out_pre"] = (e12_value(e12_codes(g.to(BF16))), None, "dg_e12")
        v = y
    elif c.out_pre:
        out["out_pre"] = (R(v), s, "bf16")
        v = R(v)
    if c.act == ACT_GELU:
        v = gelu(v) if exact else kernel_gelu_and_grad(v)[0]
    elif c.act == ACT_GELU_GRAD:
        g = gelu_grad(d.get("aux", device).to(dt)) if exact else kernel_gelu_grad(d.get("aux", device).to(dt))
        v = v * g
        if exact:
            s = s * g.abs()
    elif c.act in (ACT_MUL_AUX, ACT_MUL_AUX_U8, ACT_MUL_AUX_E12):
        a = _aux_value(c, d, device, dt)
        v = v * a
        if exact:
            s = s * a.abs()
    elif c.act == ACT_ADD_AUX:
        a = _aux_value(c, d, device, dt)
        v = v + a
        if exact:
            s = s + a.abs()
    if c.residual:
        r = d.get("res", device).to(dt)
        v = v + r
        if exact:
            s = s + r.abs()
    if c.out_f32:
        out["out_f32"] = (v, s, "f32" + fold_cls)
    if c.out_bf16:
        out["out_bf16"] = (R(v), s, "bf16" + fold_cls)
    if c.fold == "producer":   # [N/128, M, 2]: (sum, sum of squares) of the fp32 result over each 128-column slice
        x = v.view(M, N // 128, 128)
        sums = torch.stack([x.sum(-1).T, (x * x).sum(-1).T], dim=-1)
        if exact:
            sv = s.view(M, N // 128, 128)
            out["row_sums"] = (sums, torch.stack([sv.sum(-1).T, (x * x).sum(-1).T], dim=-1), "row_sums")
        else:
            out["row_sums"] = (sums, None, "row_sums")
    return out


def reference(c: Case, device="cpu", cache=None, given=None):
    return _run(c, device, True, cache, given)


def restate(c: Case, device="cpu", cache=None):
    return _run(c, device, False, cache)


def judge(got, ref, s):
    """e = |got - ref| / max(|ref|, 2^-10 s) per element (0 where got == ref, inf where the reference is an exact zero that was missed or
    got is not finite) -> (worst e, flat index of the worst element); only these two scalars leave the device"""
    got = got.double()
    diff = (got - ref).abs()
    den = torch.maximum(ref.abs(), s * 2.0 ** -10)
    e = torch.where(diff == 0, torch.zeros_like(diff), diff / den)
    e = torch.nan_to_num(e, nan=float("inf"), posinf=float("inf"))
    idx = int(e.argmax())
    return float(e.flatten()[idx]), idx


def judge_mask(got, ref, s, bound):
    """the elements whose e exceeds `bound`"""
    diff = (got.double() - ref).abs()
    e = torch.where(diff == 0, torch.zeros_like(diff), diff / torch.maximum(ref.abs(), s * 2.0 ** -10))
    return ~(e <= bound)


def u8_derived_bound(pre_ref):
    """The one-byte code's derived bound per element (test_gemm256_epilogue_kinds' condition): half a step, plus what one bf16 ulp of the
    pre-activation moves gelu' by (|gelu''| <= 0.8; ulp(x) <= 2^-7 |x|), plus 2^-20 for the fp32 arithmetic of code and decode."""
    return 0.5 * GELUQ_STEP + 0.8 * 2.0 ** -7 * pre_ref.abs() + 2.0 ** -20


def rel_err(a, b):
    """the whole-matrix figure of tests/test_ops_gpu.py"""
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------ case lists
def _kind_case(kind, M, N, K, bias, rank, **kw):
    f = dict(M=M, N=N, K=K, bias=bias, rank=rank, **kw)
    return {
        "BF16": lambda: Case(out_bf16=True, **f),
        "F32": lambda: Case(out_f32=True, **f),
        "GELU": lambda: Case(act=ACT_GELU, out_bf16=True, **f),
        "GELU_SAVE": lambda: Case(act=ACT_GELU_SAVE_GRAD, out_bf16=True, **f),
        "GELU_SAVE_U8": lambda: Case(act=ACT_GELU_SAVE_GRAD_U8, out_bf16=True, **f),
        "GELU_SAVE_12": lambda: Case(act=ACT_GELU_SAVE_GRAD_E12, out_bf16=True, **f),
        "MUL_AUX": lambda: Case(act=ACT_MUL_AUX, out_bf16=True, **f),
        "MUL_AUX_U8": lambda: Case(act=ACT_MUL_AUX_U8, out_bf16=True, **f),
        "MUL_AUX_12": lambda: Case(act=ACT_MUL_AUX_E12, out_bf16=True, **f),
        "ADD_AUX": lambda: Case(act=ACT_ADD_AUX, out_bf16=True, **f),
        "RES_F32": lambda: Case(residual=True, out_f32=True, **f),
        "RES_F32_DROP": lambda: Case(residual=True, out_f32=True, drop=0.1, **f),
        "GENERIC": lambda: Case(act=ACT_GELU_GRAD, residual=True, out_f32=True, out_bf16=True, **f),
    }[kind]()


KINDS_256 = ("BF16", "F32", "GELU", "GELU_SAVE", "GELU_SAVE_U8", "GELU_SAVE_12", "MUL_AUX", "MUL_AUX_U8", "MUL_AUX_12", "ADD_AUX", "RES_F32",
             "RES_F32_DROP", "GENERIC")
BASE_M, BASE_N = 7 * 256 + 5, 4096      # 8 x 16 = exactly 128 tiles, 5 live rows in the last m-tile; 16 column tiles = groups 6, 6, 4


def cases_256_kinds():
    """every kind x bias x rank-8 update kernel_ptr instantiates, K = 256 (nk = 4, the pipeline's minimum) and K = 384 (nk = 6)"""
    return [(kind, _kind_case(kind, BASE_M, BASE_N, K, bias, rank)) for K in (256, 384) for bias in (False, True) for rank in (False, True)
            for kind in KINDS_256]


def cases_256_fold():
    return [("RES_F32_COPY", Case(BASE_M, BASE_N, 256, bias=True, residual=True, out_f32=True, out_bf16=True, fold="producer")),
            ("ROWNORM_GELU", Case(BASE_M, BASE_N, 256, act=ACT_GELU_SAVE_GRAD, bias=True, out_bf16=True, fold="consumer")),
            ("ROWNORM_GELU", Case(BASE_M, BASE_N, 256, act=ACT_GELU_SAVE_GRAD, bias=True, out_bf16=True, fold="consumer", unfolded=True))]


def cases_256_scaled():
    """the GELU forms with pre-activations x4 and x0.05"""
    return [(kind, _kind_case(kind, BASE_M, BASE_N, 256, True, False, scale=sc)) for sc in (4.0, 0.05) for kind in ("GELU", "GELU_SAVE", "GELU_SAVE_U8", "GELU_SAVE_12")]


def cases_256_strided():
    """one case per output type, every leading dimension wider than its row and no multiple of 64 elements"""
    return [(kind, _kind_case(kind, BASE_M, BASE_N, 256, True, True, strided=True))
            for kind in ("BF16", "F32", "GELU_SAVE", "GELU_SAVE_U8", "GELU_SAVE_12", "MUL_AUX", "MUL_AUX_U8", "MUL_AUX_12", "RES_F32_DROP", "GENERIC")] + \
           [("GENERIC", Case(BASE_M, BASE_N, 256, act=ACT_GELU, bias=True, rank=True, out_pre=True, out_f32=True, out_bf16=True, strided=True))]


def cases_256_order(cus):
    """tile order and the persistent loop: fewer column tiles than the W-stationary group; tiles = CUs + tiles_n (some workgroup does two);
    M = 1024 exactly"""
    out = [("GELU_SAVE", _kind_case("GELU_SAVE", 43 * 256 + 5, 768, 256, True, False)),
           ("RES_F32", _kind_case("RES_F32", 43 * 256 + 5, 768, 256, True, False))]
    tn = 4                                                   # N = 1024: tiles_m = ceil(CUs / 4) + 1 -> tiles >= CUs + tiles_n
    tm = max(-(-(cus + tn) // tn), 32)                       # (and >= 128 tiles on any device)
    out += [("BF16", _kind_case("BF16", (tm - 1) * 256 + 5, tn * 256, 256, True, True)),
            ("GENERIC", _kind_case("GENERIC", (tm - 1) * 256 + 5, tn * 256, 256, True, False))]
    out += [("BF16", _kind_case("BF16", 1024, 8192, 256, True, False)), ("MUL_AUX", _kind_case("MUL_AUX", 1024, 8192, 256, False, False))]
    return out


def threshold_pairs():
    """(below, at): the same draws (seeded by the LARGER shape's operands, cut) on both sides of a routing threshold"""
    m127, m128 = 126 * 256 + 5, 127 * 256 + 5                                                                                   # N = 256: 127 | 128 tiles
    return [(_kind_case("GELU_SAVE", 1023, 8192, 256, True, True, draw_M=1024), _kind_case("GELU_SAVE", 1024, 8192, 256, True, True)),      # M >= 1024
            (_kind_case("RES_F32", m127, 256, 256, True, False, draw_M=m128), _kind_case("RES_F32", m128, 256, 256, True, False))]


def _c128(M, N, K, **kw):
    return Case(M, N, K, **kw)


def cases_128():
    """store_row16 at ragged N (N = 16, 48, 144: no full 128-column tile or a ragged one beside a full one), M in {1, 77, 129, 300},
    K in {64, 192}: every branch once, and the combinations listed in the GPU module's docstring"""
    G = dict(act=ACT_GELU_SAVE_GRAD, out_bf16=True)
    L = [
        _c128(1, 16, 64, out_f32=True),
        _c128(77, 48, 192, out_bf16=True, bias=True),
        _c128(129, 144, 64, act=ACT_GELU, out_bf16=True, bias=True),                                       # gelu of the fp32 value
        _c128(300, 144, 192, act=ACT_GELU, out_pre=True, out_bf16=True, bias=True),                         # out_pre with ACT_GELU: gelu of the rounded value
        _c128(77, 144, 64, out_pre=True, out_f32=True, bias=True),                                         # out_pre with ACT_NONE
        _c128(300, 48, 64, out_pre=True, out_bf16=True),
        _c128(129, 48, 192, bias=True, **G),
        _c128(300, 144, 64, bias=True, drop=0.1, **G),                                                     # dropout with GELU_SAVE_GRAD
        _c128(77, 16, 192, act=ACT_GELU_SAVE_GRAD_U8, out_bf16=True, bias=True),
        _c128(300, 144, 192, act=ACT_GELU_SAVE_GRAD_U8, out_bf16=True, out_f32=True, bias=True, rank=True),
        _c128(129, 16, 64, act=ACT_GELU_SAVE_GRAD_E12, out_bf16=True, bias=True),
        _c128(300, 144, 192, act=ACT_GELU_SAVE_GRAD_E12, out_bf16=True, bias=True, out_f32=True),
        _c128(77, 144, 192, drop=0.1, residual=True, out_f32=True, bias=True),                             # dropout with residual
        _c128(129, 48, 64, drop=0.5, out_bf16=True),                                                       # dropout alone: exact zeros
        _c128(300, 144, 64, act=ACT_GELU_GRAD, residual=True, out_f32=True, out_bf16=True),                # GELU_GRAD + residual + both outputs
        _c128(1, 48, 192, act=ACT_GELU_GRAD, out_bf16=True, bias=True),
        _c128(77, 144, 64, act=ACT_MUL_AUX, out_bf16=True),
        _c128(129, 144, 192, act=ACT_ADD_AUX, out_bf16=True, out_f32=True, bias=True),
        _c128(300, 16, 64, act=ACT_MUL_AUX_U8, out_bf16=True),                                             # N % 16: the byte form's minimum
        _c128(77, 144, 192, act=ACT_MUL_AUX_U8, out_f32=True, residual=True, bias=True),
        _c128(129, 16, 64, act=ACT_MUL_AUX_E12, out_bf16=True),                                            # N % 8 (and % 16 of the kernel)
        _c128(300, 144, 192, act=ACT_MUL_AUX_E12, out_bf16=True, rank=True),
        _c128(300, 144, 192, out_bf16=True, bias=True, rank=True),                                         # rank-8 with bias
        _c128(1, 144, 64, out_f32=True, rank=True),
        _c128(300, 256, 192, out_bf16=True, out_f32=True, bias=True, rank=True, strided=True),
        _c128(129, 144, 64, act=ACT_GELU_GRAD, residual=True, out_f32=True, out_bf16=True, bias=True, strided=True),
        _c128(300, 256, 64, scale=4.0, bias=True, **G),
        _c128(300, 256, 64, scale=0.05, bias=True, **G),
    ]
    return L


def cases_128_splitk():
    """split_k in {2, 4} accumulating onto a non-zero output; K = 192 with split 2 has a tile count the split does not divide"""
    return [_c128(77, 48, 192, out_f32=True, split_k=2), _c128(300, 144, 192, out_f32=True, split_k=2, bias=True, rank=True),
            _c128(129, 256, 256, out_f32=True, split_k=4), _c128(1, 16, 192, out_f32=True, split_k=4)]


def cases_128_hole():
    """K hole at the start, in the middle and at the end; one tile long and K - 64 long"""
    out = []
    for K in (192, 256):
        for k0, ln in ((0, 64), (64, 64), (K - 64, 64), (0, K - 64), (64, K - 64)):
            out.append(_c128(77 if K == 192 else 300, 144, K, out_f32=True, out_bf16=True, bias=True, hole=(k0, ln)))
    out.append(Case(1797, 4096, 256, out_bf16=True, bias=True, hole=(64, 64)))   # a 256x256-sized shape: the hole keeps it on the 128x128 kernel
    return out


NT_SPLITK_SHAPES = [(M, 256, K) for M in (1, 40, 300) for K in (512, 640)]
TN_SPLITK_SHAPES = [(256, 256, 256), (384, 256, 512), (640, 512, 256)]


def all_epilogue_cases(cus=256):
    """every Case of the GPU module (the CPU measurement walks the same list; shapes sized from the CU count use `cus`)"""
    L = [c for _, c in cases_256_kinds()] + [c for _, c in cases_256_fold()] + [c for _, c in cases_256_scaled()] + [c for _, c in cases_256_strided()]
    L += [c for _, c in cases_256_order(cus)]
    for a, b in threshold_pairs():
        L += [a, b]
    return L + cases_128() + cases_128_splitk() + cases_128_hole()


# ------------------------------------------------------------------------------------------------ split-K workspace paths, column sums
def nt_splitk_operands(M, N, K):
    g = torch.Generator().manual_seed(50000 + 131 * M + 7 * N + K)
    A = (torch.randn(M, K, generator=g) + 0.05).to(BF16)
    W = (torch.randn(N, K, generator=g) * (1.3 / math.sqrt(K)) + 0.02 / math.sqrt(K)).to(BF16)
    return A, W, torch.randn(M, N, generator=g) * 2.0 - 0.3


def tn_splitk_operands(M, Na, Nb):
    g = torch.Generator().manual_seed(70000 + 131 * M + 7 * Na + Nb)
    A = (torch.randn(M, Na, generator=g) * 0.5 + 0.05).to(BF16)
    B = (torch.randn(M, Nb, generator=g) * (2.6 / math.sqrt(M)) - 0.02 / math.sqrt(M)).to(BF16)
    return A, B, torch.randn(Na, Nb, generator=g) * 2.0 - 0.3, torch.randn(Na, generator=g) * 3.0 + 0.5


def product(X, Y, prev, exact):
    """X [m, k] . Y [n, k]^T (+ prev): exact -> (fp64 value, s), else the fp32 restatement"""
    if exact:
        v, s = X.double() @ Y.double().T, X.double().abs() @ Y.double().abs().T
        return (v + prev.double(), s + prev.double().abs()) if prev is not None else (v, s)
    v = X.float() @ Y.float().T
    return v + prev if prev is not None else v


def colsum(X, prev, exact):
    """column sums of X [m, c] (+ prev)"""
    if exact:
        v, s = X.double().sum(0), X.double().abs().sum(0)
        return (v + prev.double(), s + prev.double().abs()) if prev is not None else (v, s)
    v = X.float().sum(0)
    return v + prev if prev is not None else v


TRANSPOSE_COLSUM_SHAPES = [(300, 256, 0), (300, 264, 8), (1500, 128, 0), (1024, 64, 8)]   # (R, C, ld_extra): fast64 | fast64 strided | fast256 ragged | fast256


def transpose_operand(R, C, ld_extra):
    g = torch.Generator().manual_seed(90000 + 131 * R + 7 * C + ld_extra)
    return (torch.randn(R, C + ld_extra, generator=g) * 1.5 + 0.2).to(BF16), torch.randn(C, generator=g) * 3.0 + 0.5


def measure_splitk(log=None):
    """worst e of the fp32 restatement of the split-K workspace paths and of the column sums (class f32_acc)"""
    worst = 0.0
    for M, N, K in NT_SPLITK_SHAPES:
        A, W, prev = nt_splitk_operands(M, N, K)
        for acc in (False, True):
            r, s = product(A, W, prev if acc else None, True)
            e, _ = judge(product(A, W, prev if acc else None, False), r, s)
            worst = max(worst, e)
            if log:
                log(f"{'nt_splitk %dx%dx%d acc=%d' % (M, N, K, acc):70s} out_f32   f32_acc       e = {e:.4e}")
    for M, Na, Nb in TN_SPLITK_SHAPES:
        A, B, prev, cprev = tn_splitk_operands(M, Na, Nb)
        for acc in (False, True):
            r, s = product(A.T, B.T, prev if acc else None, True)
            e, _ = judge(product(A.T, B.T, prev if acc else None, False), r, s)
            worst = max(worst, e)
            if log:
                log(f"{'tn_splitk %dx%dx%d acc=%d' % (M, Na, Nb, acc):70s} out_f32   f32_acc       e = {e:.4e}")
        r, s = colsum(A, cprev, True)
        e, _ = judge(colsum(A, cprev, False), r, s)
        worst = max(worst, e)
        if log:
            log(f"{'tn_splitk %dx%dx%d' % (M, Na, Nb):70s} colsum    f32_acc       e = {e:.4e}")
    for R, C, ldx in TRANSPOSE_COLSUM_SHAPES:
        x, cprev = transpose_operand(R, C, ldx)
        r, s = colsum(x[:, :C], cprev, True)
        e, _ = judge(colsum(x[:, :C], cprev, False), r, s)
        worst = max(worst, e)
        if log:
            log(f"{'transpose_colsum %dx%d+%d' % (R, C, ldx):70s} colsum    f32_acc       e = {e:.4e}")
    return worst


CLASSES = ("bf16", "f32", "f32_acc", "dg_bf16", "dg_u8", "dg_e12", "row_sums", "bf16_mid", "f32_mid", "bf16_gg", "f32_gg", "bf16_fold", "dg_bf16_fold")


def measure_restatement(cases, log=None):
    """worst e of restate against the fp64 reference per output class, on the CPU"""
    worst = {k: 0.0 for k in CLASSES}
    ref_cache, res_cache = {}, {}
    for c in cases:
        ref = reference(c, "cpu", ref_cache)
        got = restate(c, "cpu", res_cache)
        for name, (g, _, cls) in got.items():
            r, s, _ = ref[name]
            e, _ = judge(g, r, s)
            worst[cls] = max(worst[cls], e)
            if log:
                log(f"{c.id:70s} {name:9s} {cls:13s} e = {e:.4e}")
    return worst


def parse_constants():
    """the routing constants, read from the source text"""
    def text(name):
        with open(os.path.join(ROOT, "clibd_amd", "csrc", name)) as f:
            return f.read()
    g256, g128 = text("gemm256.hip"), text("gemm.hip")
    m = re.search(r"constexpr int T_M = (\d+), T_N = (\d+), T_K = (\d+);", g256)
    b = re.search(r"constexpr int BM = (\d+), BN = (\d+), BK = (\d+);", g128)
    thr = re.search(r"if \(p\.M < (\d+) \|\| tiles < (\d+)\) return false;", g256)
    grp = re.search(r"#ifndef CLIBD_WS_GROUP\s*\n#define CLIBD_WS_GROUP (\d+)", g256)
    nkmin = re.search(r"if \(p\.K % T_K != 0 \|\| nk < (\d+) \|\| \(nk & 1\)\) return false;", g256)
    sk = re.search(r"if \(q\.K % T_K != 0 \|\| nk < (\d+) \|\| \(nk & 1\) \|\| q\.N % T_N != 0 \|\| q\.M < 1\) return 0;", g256)
    return dict(T=tuple(int(x) for x in m.groups()), B=tuple(int(x) for x in b.groups()), min_m=int(thr.group(1)), min_tiles=int(thr.group(2)),
                ws_group=int(grp.group(1)), nk_min=int(nkmin.group(1)), splitk_nk_min=int(sk.group(1)))
