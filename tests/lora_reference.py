"""CPU-importable half of the LoRA adapter kernel form tests (tests/test_lora_forms_gpu.py, tests/test_lora_forms_cpu.py).

Holds, for the five entries of clibd_amd/csrc/lora.hip (lora_pack, lora_down_proj, lora_workspace_bytes, lora_wgrad, lora_backward):

* the operations in fp64 from the same bf16 operands, each with `s`, the fp64 sum of magnitudes of everything added to make an element:
  the four images of lora_pack, t = x . a_cat^T, dt = [dq B_q | dv B_v | 0 x 8], and the four gradients as include/clibd_hip.h states them
  (dB_q[n,r] += sum_m dq[m,n] t[m,r], dB_v[n,r] += sum_m dv[m,n] t[m,4+r], dA_q[r,k] += sum_m dt[m,r] x[m,k], dA_v[r,k] += sum_m dt[m,4+r] x[m,k]);
* the same in fp32 torch with the kernels' rounding points: bf16 operands, fp32 accumulation, ONE bf16 rounding of t and of dt, and the
  gradients summed in the kernels' own units: the VALU kernel's 256-row blocks (four row groups, added in group order, blocks added onto the
  output), the MFMA kernels' 32-row slabs accumulated in sequence per workgroup (slabs first, first + G, ...), the workgroups' copies then added
  by lora_reduce_kernel's four chains of four (bit for bit its order) or, for the atomic forms, in ascending order (any order is a legal one);
  the gradients of lora_backward are taken from the ROUNDED dt, as the kernels take them from the dt they stored;
* the judgement: gemm_reference.judge (e = |got - ref| / max(|ref|, 2^-10 s)), and `locate_*`, which name the matrix, the column segment
  (`which`, `half`), the 64-column tile, wave and lane group of an element for the MFMA forms and the column thread and its row groups' waves for the VALU form;
* `route`: the Python mirror of the host routing of clibd_lora_wgrad / clibd_lora_backward, every constant read from lora.hip (parse_constants);
* the operands (`draw`) and the case lists both test modules walk.  Operands of M H <= 2^22 elements are drawn on the host, so the CPU module
  restates the very bits the GPU module launches; larger ones are drawn on the device that runs the case (the same seeds and distributions, other
  bits), so the CPU measurement of those cases is over its own draws of the same cases."""
import os
import re
from dataclasses import dataclass

import torch

from gemm_reference import BF16, F32, F64, bfr, judge, judge_mask, rel_err  # noqa: F401  (one judgement for both form modules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# routing constants of lora.hip (test_lora_forms_cpu.py checks each against the source text)
LW_ROWS = 256                  # rows per block of lora_wgrad_kernel
LWM_ROWS = 32                  # rows per slab of the MFMA kernels
MFMA_MIN_M = 8192              # without a workspace the MFMA form of lora_wgrad needs this many rows
FUSED_MIN_M = 131072           # lora_backward's fused pair
TILES_SET = (1, 2, 3, 4, 5, 6, 7, 8)   # H / 128 with an instantiation of lora_wgrad_mfma_kernel
NCH_SET = (4, 6, 8)            # 2H / 256 with an instantiation of lora_dt_db_kernel
DOWN_PROJ_MAX_BLOCKS = 2048
H_MAX = 1024
CLASSES = ("t", "dt_gemm", "dt_fused", "g_valu", "g_mfma_atomic", "g_mfma_partials")
GRADS = ("dA_q", "dA_v", "dB_q", "dB_v")


# ------------------------------------------------------------------------------------------------ routing mirror
def workspace_bytes(M, H, cus):
    """clibd_lora_workspace_bytes"""
    if M <= 0 or H <= 0 or M % LWM_ROWS or H % 128:
        return 0
    return min(cus, M // LWM_ROWS) * 16 * H * 4


def _lcm(nch):
    return nch if nch % 4 == 0 else (2 * nch if nch % 2 == 0 else 4 * nch)


def _per_wg(nslab, groups):
    """(fewest, most) slabs of a workgroup that walks slabs first, first + groups, ..."""
    return nslab // groups, -(-nslab // groups)


def route(entry, M, H, workspace, cus):
    """Which kernels a call of clibd_lora_wgrad ("wgrad") / clibd_lora_backward ("backward") launches.  `workspace`: a non-null workspace
    pointer is passed.  Returns form ("valu" | "mfma" | "fused"), kernels, grid, tiles / nch / lcm, slabs per workgroup (fewest, most) of each
    MFMA kernel, the copy counts (g_b, g_a) lora_reduce_kernel adds (0, 0 without a workspace or in the VALU form) and the bytes of the
    workspace the kernels write (copies x 16 H floats)."""
    assert entry in ("wgrad", "backward") and M > 0 and 0 < H <= H_MAX and H % 64 == 0
    nslab = M // LWM_ROWS
    r = dict(entry=entry, tiles=None, nch=None, lcm=None, g_b=0, g_a=0, used_bytes=0, ws_bytes=workspace_bytes(M, H, cus))
    nch = 2 * H // 256
    if entry == "backward" and M % LWM_ROWS == 0 and M >= FUSED_MIN_M and H % 256 == 0 and nch in NCH_SET:
        gb, ga = min(cus, nslab), min((2 * cus + 1) // 2, nslab)
        r.update(form="fused", kernels=(f"lora_dt_db_kernel<{nch}>", f"lora_wgrad_mfma_kernel<{H // 128}>") + (("lora_reduce_kernel",) if workspace else ()),
                 grid=((gb,), (ga, 2)), tiles=H // 128, nch=nch, lcm=_lcm(nch), slabs_per_wg=(_per_wg(nslab, gb), _per_wg(nslab, ga)))
        if workspace:
            r.update(g_b=gb, g_a=ga, used_bytes=max(gb, ga) * 16 * H * 4)
        return r
    pre = ("gemm_bf16_nt_kernel (k hole)",) if entry == "backward" else ()
    if M % LWM_ROWS == 0 and (M >= MFMA_MIN_M or workspace) and H % 128 == 0 and H // 128 in TILES_SET:
        groups = min((2 * cus + 5) // 6, nslab)
        r.update(form="mfma", kernels=pre + (f"lora_wgrad_mfma_kernel<{H // 128}>",) + (("lora_reduce_kernel",) if workspace else ()),
                 grid=((groups, 6),), tiles=H // 128, slabs_per_wg=(_per_wg(nslab, groups),))
        if workspace:
            r.update(g_b=groups, g_a=groups, used_bytes=groups * 16 * H * 4)
        return r
    r.update(form="valu", kernels=pre + ("lora_wgrad_kernel",), grid=((-(-M // LW_ROWS),),), slabs_per_wg=())
    return r


def valu_lds_bytes(H):
    return (3 * (H // 4) * 16 + 4 * H + (4 * H) // 32 + 32) * 4


def down_proj_blocks(M):
    return min((M + 3) // 4, DOWN_PROJ_MAX_BLOCKS)


def parse_constants():
    """the routing constants, read from the text of lora.hip"""
    with open(os.path.join(ROOT, "clibd_amd", "csrc", "lora.hip")) as f:
        src = f.read()
    one = lambda pat: re.search(pat, src)
    wg = one(r"if \(M % LWM_ROWS == 0 && \(M >= (\d+) \|\| workspace != nullptr\) && H % 128 == 0 && ld_dt % 8 == 0\)")
    fused = one(r"const bool fused = M % LWM_ROWS == 0 && M >= (\d+) && H % 256 == 0 && \(nch == 4 \|\| nch == 6 \|\| nch == 8\);")
    launch = src[src.index("#define LWM_LAUNCH(T)"):src.index("#undef LWM_LAUNCH")]
    launch2 = src[src.index("#define LWM_LAUNCH2(T)"):src.index("#undef LWM_LAUNCH2")]
    ldb = src[src.index("#define LDB_LAUNCH(N_)"):src.index("#undef LDB_LAUNCH")]
    return dict(
        lw_rows=int(one(r"constexpr int LW_ROWS = (\d+);").group(1)), lwm_rows=int(one(r"constexpr int LWM_ROWS = (\d+);").group(1)),
        mfma_min_m=int(wg.group(1)), fused_min_m=int(fused.group(1)),
        tiles=tuple(sorted(int(x) for x in re.findall(r"LWM_LAUNCH\((\d)\);", launch))),
        tiles_fused=tuple(sorted(int(x) for x in re.findall(r"LWM_LAUNCH2\((\d)\);", launch2))),
        nch=tuple(sorted(int(x) for x in re.findall(r"LDB_LAUNCH\((\d)\);", ldb))),
        want_wgrad=one(r"const int want = \(2 \* num_cus \+ 5\) / 6;") is not None,
        want_fused_a=one(r"const int want = \(2 \* num_cus \+ 1\) / 2;") is not None,
        groups_fused_b=one(r"const int groups = num_cus < nslab \? num_cus : nslab;") is not None,
        ws_copies=one(r"const int g = lora_num_cus\(\) < M / 32 \? lora_num_cus\(\) : M / 32;\s*\n\s*return \(size_t\)g \* 16 \* \(size_t\)H \* sizeof\(float\);") is not None,
        ws_zero=one(r"if \(M <= 0 \|\| H <= 0 \|\| M % 32 != 0 \|\| H % 128 != 0\) return 0;") is not None,
        valu_blocks=one(r"const int blocks = \(M \+ LW_ROWS - 1\) / LW_ROWS;") is not None,
        valu_lds=one(r"const size_t lds = \(\(size_t\)3 \* \(H / 4\) \* 16 \+ \(size_t\)4 \* H \+ \(size_t\)\(4 \* H\) / 32 \+ 32\) \* sizeof\(float\);") is not None,
        lcm=one(r"constexpr int LCM = \(NCH % 4 == 0\) \? NCH : \(NCH % 2 == 0 \? 2 \* NCH : 4 \* NCH\);") is not None,
        six_steps=one(r"slab \+= 6 \* G\)") is not None and len(re.findall(r"^\s*LWM_STEP\(slab", src, re.M)) == 6,
        ring=int(one(r"constexpr int RING = (\d+);").group(1)),
        down_cap=int(one(r"if \(blocks > (\d+)\) blocks = \1;").group(1)),
        h_max=int(one(r"H % 64 != 0 \|\| H > (\d+)\) return set_error\(CLIBD_EINVAL, \"lora_wgrad").group(1)),
    )


# ------------------------------------------------------------------------------------------------ where an element is computed
def locate_mfma(name, H, idx):
    """segment, tile, wave and lanes of flat element `idx` of gradient `name` in lora_wgrad_mfma_kernel (dB also: lora_dt_db_kernel's chunk)"""
    if name.startswith("dB"):
        col, r = divmod(idx, 4)
        which, c = (0, r) if name == "dB_q" else (1, 4 + r)
        el = f"{name}[n = {col}, r = {r}]"
    else:
        r, col = divmod(idx, H)
        which, c = 2, (8 if name == "dA_q" else 12) + r
        el = f"{name}[r = {r}, k = {col}]"
    half, cc = divmod(col, H // 2)
    tl = cc // 64
    return (f"{el}: segment which = {which} ({('dq', 'dv', 'x')[which]}), half = {half}, 64-column tile {tl} (wave {tl % 4}, its tile {tl // 4}), "
            f"16-column group d = {cc % 64 // 16}, lane group g = {cc % 16 // 4} (lanes {16 * (cc % 16 // 4) + c}), accumulator slot {cc % 4}, MFMA column c = {c}; "
            f"fused dt/dB kernel: 256-column chunk {(col + (H if which == 1 else 0)) // 256}, wave {col % 256 // 64}")


def locate_valu(name, H, idx):
    """column thread and row-group waves of flat element `idx` of gradient `name` in lora_wgrad_kernel"""
    if name.startswith("dB"):
        col, r = divmod(idx, 4)
        el = f"{name}[n = {col}, r = {r}]"
    else:
        r, col = divmod(idx, H)
        el = f"{name}[r = {r}, k = {col}]"
    ct, ch = col // 4, H // 4
    return (f"{el}: column thread ct = {ct} (column slot {col % 4}), row groups 0..3 = threads {ct}, {ch + ct}, {2 * ch + ct}, {3 * ch + ct} "
            f"(wavefronts {ct // 64}, {(ch + ct) // 64}, {(2 * ch + ct) // 64}, {(3 * ch + ct) // 64}); output image index {idx} (atomic by thread {idx % H} of its block)")


def locate_rows(what, m, n, cus=None, M=None):
    """row-indexed outputs (t, dt): slab, loading wave, and for the fused kernel the workgroup"""
    s = f"{what}[m = {m}, column {n}]: 32-row slab {m // 32}, row {m % 32} of it (loaded by wave {m % 32 // 8}), 256-row block {m // 256}, row group {m % 4}"
    if cus and M and M % 32 == 0:
        g = min(cus, M // 32)
        s += f"; fused kernel: workgroup {m // 32 % g}, its slab {m // 32 // g}"
    return s


# ------------------------------------------------------------------------------------------------ operands
def gen_device(M, H, device):
    """small draws are made on the host (the CPU module restates exactly these); large ones on `device` from the same seeds"""
    return torch.device("cpu") if M * H <= (1 << 22) else torch.device(device)


def draw(M, H, mode, seed, device, kinds=("dqkv", "x", "t", "dt", "init")):
    """Seeded operands of one call as a dict.  mode "real": dqkv ~ N(0.01, 0.1) (the engine's gradient scale; its k segment is NaN: nothing may
    read it), x ~ N(0.05, 1), t ~ N(0.1, 1) x (1 + r / 8) per rank r, dt ~ N(-0.01, 0.1) x (1 + r / 8) (columns 8.. are the caller's padding).
    mode "int": independent draws from {-2 .. 2} with a different skew per tensor and per rank, so that every fp32 partial sum of the gradients
    is an exact integer at these M (|sum| <= 4 M + 8 < 2^24 for M <= 2^21) and no two segments, operands or ranks are exchangeable.
    init: what the four gradients hold before the call (non-zero: the accumulate contract)."""
    gd = gen_device(M, H, device)
    out = {}
    rank = 1.0 + torch.arange(8, dtype=F32, device=gd) / 8.0
    for i, k in enumerate(("dqkv", "x", "t", "dt", "init")):
        if k not in kinds:
            continue
        g = torch.Generator(device=gd).manual_seed(7_000_003 * seed + 104_729 * i + 31 * M + H + (0 if mode == "real" else 555))
        rn = lambda *shape: torch.randn(*shape, generator=g, device=gd)
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g, device=gd).to(F32)
        if mode == "real":
            if k == "dqkv":
                v = rn(M, 3 * H) * 0.1 + 0.01
            elif k == "x":
                v = rn(M, H) + 0.05
            elif k == "t":
                v = (rn(M, 8) + 0.1) * rank
            elif k == "dt":
                v = (rn(M, 8) * 0.1 - 0.01) * rank
            else:
                v = [rn(4, H) * 2.0 + 0.3, rn(4, H) * 2.0 - 0.3, rn(H, 4) * 2.0 + 0.5, rn(H, 4) * 2.0 - 0.5]
        else:
            if k == "dqkv":
                v = ri(-2, 2, M, 3 * H)
                v[:, 2 * H:] = torch.where(v[:, 2 * H:] == -2, torch.ones((), device=gd), v[:, 2 * H:])           # dv: no -2, more +1
            elif k == "x":
                v = torch.where((u := ri(-2, 2, M, H)) == 2, -torch.ones((), device=gd), u)                       # x: no +2, more -1
            elif k == "t":
                v = ri(-2, 2, M, 8)
                v = torch.where(v == (torch.arange(8, device=gd) % 5 - 2).to(F32), torch.zeros((), device=gd), v)  # rank r never takes the value r % 5 - 2
            elif k == "dt":
                v = ri(-2, 2, M, 8)
                v = torch.where(v == ((torch.arange(8, device=gd) + 2) % 5 - 2).to(F32), torch.ones((), device=gd), v)
            else:
                v = [ri(-8, 8, 4, H) + 1, ri(-8, 8, 4, H) - 1, ri(-8, 8, H, 4) + 2, ri(-8, 8, H, 4) - 2]
        if k == "dqkv":
            v[:, H:2 * H] = float("nan")
        out[k] = [t.to(device) for t in v] if k == "init" else v.to(BF16).to(device)
    return out


def draw_adapter(H, mode, seed, device):
    """fp32 adapter parameters a_q, a_v [4, H], b_q, b_v [H, 4].  real: N(0, 1) / N(0, 0.2) with distinct means; int: A from {-2 .. 2}; B is +-1 at
    16 rows per rank (one per H / 16 rows, another phase per rank and per matrix) and 0 elsewhere, so that |dt| <= 32 is exact in bf16 and the
    gradients taken from it stay below 2^24."""
    g = torch.Generator().manual_seed(911 * seed + H + (0 if mode == "real" else 77))
    if mode == "real":
        p = [torch.randn(4, H, generator=g) + 0.05, torch.randn(4, H, generator=g) - 0.05, torch.randn(H, 4, generator=g) * 0.2 + 0.01,
             torch.randn(H, 4, generator=g) * 0.2 - 0.01]
    else:
        a = [torch.randint(-2, 3, (4, H), generator=g).float(), torch.randint(-2, 2, (4, H), generator=g).float()]
        b = []
        for mat in range(2):
            w = torch.zeros(H, 4)
            for r in range(4):
                rows = (torch.arange(16) * (H // 16) + (5 * r + 3 * mat) % (H // 16))
                w[rows, r] = (torch.randint(0, 2, (16,), generator=g) * 2 - 1).float() * (1 if (r + mat) % 2 else -1)
            b.append(w)
        p = a + b
    return [t.to(device) for t in p]


# ------------------------------------------------------------------------------------------------ the operations
def pack_images(a_q, a_v, b_q, b_v):
    """the four bf16 images of lora_pack (exact: one bf16 rounding of each parameter, zeros elsewhere)"""
    H = a_q.shape[1]
    dev = a_q.device
    v_fwd = torch.zeros((3 * H, 8), dtype=BF16, device=dev)
    v_fwd[:H, :4] = b_q.to(BF16)
    v_fwd[2 * H:, 4:] = b_v.to(BF16)
    v_bwd = torch.cat([a_q.to(BF16).T, a_v.to(BF16).T], dim=1).contiguous()
    a_cat = torch.cat([a_q.to(BF16), a_v.to(BF16)], dim=0).contiguous()
    w_dt = torch.zeros((16, 3 * H), dtype=BF16, device=dev)
    w_dt[:4, :H] = b_q.to(BF16).T
    w_dt[4:8, 2 * H:] = b_v.to(BF16).T
    return v_fwd, v_bwd, a_cat, w_dt


def _chunks(M, rows=16384):
    return [(i, min(i + rows, M)) for i in range(0, M, rows)]


def t_reference(x, a_cat):
    """t = x . a_cat^T in fp64 -> (ref [M, 8], s)"""
    a = a_cat.double()
    return x.double() @ a.T, x.double().abs() @ a.abs().T


def t_restate(x, a_cat):
    return bfr(x.float() @ a_cat.float().T)


def dt_reference(dqkv, w_dt):
    """dt = [dq B_q | dv B_v | 0 x 8] in fp64 from dqkv [M, 3H] (k segment ignored) and the packed image w_dt [16, 3H] -> (ref [M, 16], s)"""
    M, H = dqkv.shape[0], dqkv.shape[1] // 3
    ref, s = torch.zeros((M, 16), dtype=F64, device=dqkv.device), torch.zeros((M, 16), dtype=F64, device=dqkv.device)
    wq, wv = w_dt[:8, :H].double(), w_dt[:8, 2 * H:].double()
    for i, j in _chunks(M):
        dq, dv = dqkv[i:j, :H].double(), dqkv[i:j, 2 * H:].double()
        ref[i:j, :8] = dq @ wq.T + dv @ wv.T
        s[i:j, :8] = dq.abs() @ wq.abs().T + dv.abs() @ wv.abs().T
    return ref, s


def dt_restate(dqkv, w_dt):
    """fp32 accumulation over the q and v segments, one bf16 rounding (the GEMM's store and the fused kernel's pack2bf alike)"""
    M, H = dqkv.shape[0], dqkv.shape[1] // 3
    out = torch.zeros((M, 16), dtype=F32, device=dqkv.device)
    out[:, :8] = dqkv[:, :H].float() @ w_dt[:8, :H].float().T + dqkv[:, 2 * H:].float() @ w_dt[:8, 2 * H:].float().T
    return bfr(out)


def grads_reference(dqkv, x, t, dt, init):
    """the four gradients in fp64, onto `init` -> {name: (ref, s)}; dt: the bf16 dt the gradients are taken from (columns 0..7 are read)"""
    M, H = x.shape
    acc = {k: [torch.zeros(sh, dtype=F64, device=x.device), torch.zeros(sh, dtype=F64, device=x.device)]
           for k, sh in (("dA_q", (4, H)), ("dA_v", (4, H)), ("dB_q", (H, 4)), ("dB_v", (H, 4)))}
    for i, j in _chunks(M):
        dq, dv, xx, tt, gg = dqkv[i:j, :H].double(), dqkv[i:j, 2 * H:].double(), x[i:j].double(), t[i:j].double(), dt[i:j, :8].double()
        for name, L, R in (("dA_q", gg[:, :4], xx), ("dA_v", gg[:, 4:8], xx), ("dB_q", dq, tt[:, :4]), ("dB_v", dv, tt[:, 4:8])):
            acc[name][0] += L.T @ R
            acc[name][1] += L.abs().T @ R.abs()
    return {k: (acc[k][0] + i0.double(), acc[k][1] + i0.double().abs()) for k, i0 in zip(GRADS, init)}


def _reduce_order(copies, init_flat):
    """lora_reduce_kernel: wave w adds copies w, w + 4, ... in four chains of four plus a scalar tail; waves meet as (p0 + p1) + (p2 + p3)"""
    G = copies.shape[0]
    part = []
    for w in range(4):
        s = [torch.zeros_like(init_flat) for _ in range(4)]
        xx = w
        while xx + 12 < G:
            for c in range(4):
                s[c] = s[c] + copies[xx + 4 * c]
            xx += 16
        while xx < G:
            s[0] = s[0] + copies[xx]
            xx += 4
        part.append((s[0] + s[1]) + (s[2] + s[3]))
    return init_flat + ((part[0] + part[1]) + (part[2] + part[3]))


def _unit_partials(L, R, rows):
    """fp32 products L^T R over consecutive units of `rows` rows (zero-padded to whole units) -> [units, L columns, R columns]"""
    M = L.shape[0]
    n = -(-M // rows)
    if n * rows != M:
        L = torch.cat([L, L.new_zeros((n * rows - M, L.shape[1]))])
        R = torch.cat([R, R.new_zeros((n * rows - M, R.shape[1]))])
    return torch.bmm(L.float().view(n, rows, -1).transpose(1, 2), R.float().view(n, rows, -1))


def _walk(P, G):
    """workgroup w accumulates units w, w + G, ... in sequence -> [G, ...] (missing units are zeros: adding them changes nothing)"""
    n = P.shape[0]
    k = -(-n // G)
    if k * G != n:
        P = torch.cat([P, P.new_zeros((k * G - n,) + P.shape[1:])])
    P = P.view(k, G, *P.shape[1:])
    acc = P[0].clone()
    for i in range(1, k):
        acc = acc + P[i]
    return acc


def grads_restate(dqkv, x, t, dt, init, form, g_b, g_a, partials):
    """the four gradients in fp32 in the kernels' units (module docstring).  form "valu": 256-row blocks; else slabs walked by g_b (dB) and g_a (dA)
    workgroups, combined in lora_reduce_kernel's order (`partials`) or in ascending order (atomics)."""
    M, H = x.shape
    dq, dv, gg = dqkv[:, :H], dqkv[:, 2 * H:], dt[:, :8]
    out = {}
    for name, L, R, i0 in (("dA_q", gg[:, :4], x, init[0]), ("dA_v", gg[:, 4:8], x, init[1]), ("dB_q", dq, t[:, :4], init[2]), ("dB_v", dv, t[:, 4:8], init[3])):
        if form == "valu":
            nb = -(-M // LW_ROWS)
            pad = nb * LW_ROWS - M
            Lp = torch.cat([L, L.new_zeros((pad, L.shape[1]))]) if pad else L
            Rp = torch.cat([R, R.new_zeros((pad, R.shape[1]))]) if pad else R
            # row group g of block b: rows 256 b + g + 4 j
            Lg = Lp.float().view(nb, LW_ROWS // 4, 4, -1).permute(0, 2, 3, 1).reshape(nb * 4, L.shape[1], LW_ROWS // 4)
            Rg = Rp.float().view(nb, LW_ROWS // 4, 4, -1).permute(0, 2, 1, 3).reshape(nb * 4, LW_ROWS // 4, R.shape[1])
            P = torch.zeros((nb * 4, L.shape[1], R.shape[1]), dtype=F32, device=x.device)
            for j in range(LW_ROWS // 4):       # one row per step, as the thread walks its row group
                P = P + Lg[:, :, j, None] * Rg[:, j, None, :]
            P = P.view(nb, 4, L.shape[1], R.shape[1])
            blocks = ((P[:, 0] + P[:, 1]) + P[:, 2]) + P[:, 3]
            acc = i0.float().clone()
            for b in range(nb):
                acc = acc + blocks[b]
            out[name] = acc
        else:
            G = g_a if name.startswith("dA") else g_b
            copies = _walk(_unit_partials(L, R, LWM_ROWS), G)
            flat = copies.reshape(G, -1)
            if partials:
                out[name] = _reduce_order(flat, i0.float().reshape(-1)).view(i0.shape)
            else:
                acc = i0.float().reshape(-1).clone()
                for w in range(G):
                    acc = acc + flat[w]
                out[name] = acc.view(i0.shape)
    return out


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    entry: str            # "wgrad" | "backward"
    M: int
    H: int
    workspace: bool
    mode: str = "real"    # "real" | "int"
    ld_dt: int = 16
    ld_extra: int = 0     # ld_dqkv = 3H + ld_extra
    seed: int = 0

    @property
    def id(self):
        return f"{self.entry}-M{self.M}-H{self.H}-{'ws' if self.workspace else 'nows'}-{self.mode}-lddt{self.ld_dt}-ld+{self.ld_extra}"


def wgrad_groups(cus):
    return (2 * cus + 5) // 6


VALU_H = (64, 128, 192, 256, 320, 768, 1024)
VALU_M = (1, 3, 15, 16, 17, 255, 256, 257, 700)
MODES = ("real", "int")


def _strides(i):
    return dict(ld_dt=(8, 16, 24)[i % 3], ld_extra=(0, 8)[i % 2])


def cases_valu(H, mode):
    """every M of the VALU list at width H, without a workspace; the leading dimensions cycle through ld_dt 8 | 16 | 24 and ld_dqkv 3H | 3H + 8"""
    return [Case("wgrad", M, H, False, mode, seed=1, **_strides(i)) for i, M in enumerate(VALU_M)]


def cases_valu_routes(mode):
    """shapes that cannot take MFMA: a whole-slab M below 8192 without a workspace, a ragged M above 8192 (with a workspace pointer too), and a
    width with H % 128 == 64 at a whole-slab M with a workspace pointer"""
    return [Case("wgrad", 512, 384, False, mode, seed=2, ld_dt=8), Case("wgrad", 8192 + 7, 256, False, mode, seed=2, ld_dt=24, ld_extra=8),
            Case("wgrad", 8192 + 7, 128, True, mode, seed=2), Case("wgrad", 512, 320, True, mode, seed=2, ld_dt=8, ld_extra=8)]


def mfma_slab_counts(cus):
    G = wgrad_groups(cus)
    return (1, 5, G - 1, G, G + 1, 3 * G + 1, 5 * G + 1, 6 * G + 1, 12 * G + 5)


def cases_mfma(H, mode, cus):
    """with a workspace: the full slab list at H = 384 and 768 (slabs per workgroup 1, 1|2, 3|4, 5|6, 6|7, 12|13: every entry and exit of the six-step
    trip), a subset with a `|` pair at the other widths"""
    G = wgrad_groups(cus)
    counts = mfma_slab_counts(cus) if H in (384, 768) else (1, G + 1, 3 * G + 1) if H in (512, 1024) else (1, 5, G + 1, 3 * G + 1, 6 * G + 1)
    return [Case("wgrad", 32 * n, H, True, mode, seed=3, **_strides(i + 1)) for i, n in enumerate(counts)]


def cases_mfma_atomic(H, mode, cus):
    """without a workspace (M >= 8192): two slab counts per TILES"""
    G = wgrad_groups(cus)
    return [Case("wgrad", 32 * n, H, False, mode, seed=4, **_strides(i)) for i, n in enumerate((MFMA_MIN_M // 32, max(3 * G + 1, MFMA_MIN_M // 32 + 1)))]


MFMA_H = (128, 256, 384, 512, 640, 768, 896, 1024)
REDUCE_SLABS = (2, 3, 4, 13, 16, 17)


def cases_reduce(mode):
    """lora_reduce_kernel's chain tails: G = 2, 3, 4 (waves without a copy), 13 (first full chain round for wave 0), 16, 17"""
    return [Case("wgrad", 32 * n, 384, True, mode, seed=5) for n in REDUCE_SLABS]


def cases_backward_two_call(cus):
    G = wgrad_groups(cus)
    out = []
    for H in (384, 512, 768, 1024, 128, 256):
        out += [Case("backward", 257, H, False, "real", seed=6), Case("backward", 32 * (G + 1), H, True, "real", seed=6, ld_dt=24, ld_extra=8),
                Case("backward", 32 * (G + 1), H, True, "int", seed=6)]
    out += [Case("backward", 8192, 384, False, "real", seed=6), Case("backward", 700, 128, False, "int", seed=6), Case("backward", 8192 + 32, 640, True, "real", seed=6)]
    return out


FUSED_H = (512, 768, 1024)
FUSED_M = (FUSED_MIN_M, FUSED_MIN_M + 32)


def cases_fused(H):
    """both M with a workspace, once without, once with integers (the draws are those of the larger M, cut)"""
    return [Case("backward", FUSED_M[0], H, True, "real", seed=7), Case("backward", FUSED_M[1], H, True, "real", seed=7, ld_dt=24, ld_extra=8),
            Case("backward", FUSED_M[1], H, False, "real", seed=7), Case("backward", FUSED_M[0], H, True, "int", seed=7)]


DOWN_H = (8, 128, 512, 520, 768, 1024)
DOWN_M = (1, 3, 4, 5, 8191, 8192, 8192 + 7)
PACK_H = (64, 128, 384, 768, 1024)


def draw_down(M, H, seed=8):
    g = torch.Generator().manual_seed(1301 * seed + 17 * M + H)
    x = (torch.randn(M, H, generator=g) + 0.05).to(BF16)
    a = ((torch.randn(8, H, generator=g) + 0.02) * (1.0 + torch.arange(8)[:, None] / 8.0)).to(BF16)
    return x, a


def all_gradient_cases(cus=256, fused=False):
    L = []
    for mode in MODES:
        for H in VALU_H:
            L += cases_valu(H, mode)
        L += cases_valu_routes(mode)
        for H in MFMA_H:
            L += cases_mfma(H, mode, cus) + cases_mfma_atomic(H, mode, cus)
        L += cases_reduce(mode)
    L += cases_backward_two_call(cus)
    if fused:
        for H in FUSED_H:
            L += cases_fused(H)
    return L


def grad_class(r, workspace):
    return "g_valu" if r["form"] == "valu" else "g_mfma_partials" if workspace else "g_mfma_atomic"


# ------------------------------------------------------------------------------------------------ the CPU measurement
def operands_for(c: Case, device="cpu", draw_M=None):
    """(dqkv, x, t, dt or None, init, w_dt or None) of a case; backward: dt is an output, w_dt the packed image of the case's adapter"""
    d = draw(draw_M or c.M, c.H, c.mode, c.seed, device, kinds=("dqkv", "x", "t", "init") + (("dt",) if c.entry == "wgrad" else ()))
    M = c.M
    w_dt = pack_images(*draw_adapter(c.H, c.mode, c.seed, device))[3] if c.entry == "backward" else None
    return d["dqkv"][:M], d["x"][:M], d["t"][:M], (d["dt"][:M] if c.entry == "wgrad" else None), d["init"], w_dt


def measure_restatement(cases, cus=256, log=None):
    """worst e of the fp32 restatement against fp64 per class over the REAL-valued cases (the integer cases have no bound: they are equalities,
    and the restatement must meet them exactly too)"""
    worst = {k: 0.0 for k in CLASSES}
    for c in cases:
        r = route(c.entry, c.M, c.H, c.workspace, cus)
        dqkv, x, t, dt, init, w_dt = operands_for(c, draw_M=FUSED_M[1] if c.M >= FUSED_MIN_M else None)
        if c.entry == "backward":
            ref, s = dt_reference(dqkv, w_dt)
            dt = dt_restate(dqkv, w_dt).to(BF16)
            cls = "dt_fused" if r["form"] == "fused" else "dt_gemm"
            if c.mode == "real":
                e, _ = judge(dt.float()[:, :8], ref[:, :8], s[:, :8])
                worst[cls] = max(worst[cls], e)
                if log:
                    log(f"{c.id:64s} dt    {cls:16s} e = {e:.4e}")
            else:
                assert torch.equal(dt.double(), ref), c.id
        refs = grads_reference(dqkv, x, t, dt, init)
        g_b, g_a = (r["g_b"], r["g_a"]) if c.workspace and r["form"] != "valu" else (r["grid"][0][0], r["grid"][-1][0])
        got = grads_restate(dqkv, x, t, dt, init, r["form"], g_b, g_a, bool(c.workspace) and r["form"] != "valu")
        cls = grad_class(r, c.workspace)
        for name in GRADS:
            ref, s = refs[name]
            if c.mode == "int":
                assert torch.equal(got[name].double(), ref), (c.id, name)
                continue
            e, _ = judge(got[name], ref, s)
            worst[cls] = max(worst[cls], e)
            if log:
                log(f"{c.id:64s} {name:5s} {cls:16s} e = {e:.4e}")
    return worst


def measure_down_proj(log=None):
    worst = 0.0
    for H in DOWN_H:
        for M in DOWN_M:
            x, a = draw_down(M, H)
            ref, s = t_reference(x, a)
            e, _ = judge(t_restate(x, a), ref, s)
            worst = max(worst, e)
            if log:
                log(f"{'down_proj-M%d-H%d' % (M, H):64s} t     {'t':16s} e = {e:.4e}")
    return worst
