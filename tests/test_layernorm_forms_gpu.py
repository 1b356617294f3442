"""Every LayerNorm kernel form against an fp64 statement of the operation (GPU).

Dispatch of clibd_layernorm_fwd / clibd_layernorm_bwd, read from the host code of csrc/layernorm.hip.  N = ceil(H / 256) float4 chunks
per lane: H = 64 / 128 -> N = 1 (16 / 32 live lanes), 320 -> 2, 576 -> 3, 832 -> 4 (a 16-lane last chunk after full ones), 768 -> 3 and
1024 -> 4 (full chunks).

  forward   condition                                               instantiation                      rows per sweep   cases below
  F-plain   lora_a NULL                                             layernorm_fwd_kernel<N, false, 4>  2048*4*4 = 32768 lora=False
  F-lora    lora_a given                                            layernorm_fwd_kernel<N, true, 2>   2048*4*2 = 16384 lora=True

  backward  condition                                               instantiation                      rows per sweep   cases below
  B1        no dgamma, no dx_fp8, not (two-row)                     layernorm_bwd_kernel<N, false, 1>  4096*4   = 16384 a1 .. a8
  B2        no dgamma, no dx_fp8, two-row                           layernorm_bwd_kernel<N, false, 2>  4096*4*2 = 32768 a5, a7 at M = 131075
  PG        dgamma, no dx_fp8 (workspace: ordered, else atomic)     layernorm_bwd_kernel<N, true, 1>   1024*4   = 4096  c1, c4 (atomic), c2, c3 (ordered)
  F8-1      dx_fp8, no dgamma, not (two-row and N <= 3 and          layernorm_bwd_fp8_kernel<N, 1>     16384            d1 .. d4; d1 at M = 131075, H = 832
            dres_bf16)
  F8-2      dx_fp8, no dgamma, two-row, N <= 3, dres_bf16           layernorm_bwd_fp8_kernel<N, 2>     32768            d1, d3 at M = 131075
  F8-PG     dx_fp8 and dgamma (workspace: ordered, else atomic)     layernorm_bwd_fp8_pg_kernel<N>     4096             e1 (atomic), e2, e3 (ordered)
  two-row = dy bf16, no fp32 dres, no dx_f32, M >= 131072.

The reference is torch.nn.functional.layer_norm in float64 and its autograd, plus the residual in fp64; the backward takes (mean, rstd)
computed in fp64 and cast to fp32, so it is judged independently of the forward kernel.  Operands of M < 4096 are made and judged on the
host, larger ones on the device (torch's own fp64 kernels).  Relative errors are per row (the worst row must meet the bound)."""
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

BF16, F32, F64, FP8, U8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn, torch.uint8
HS = [64, 128, 320, 576, 768, 832, 1024]
SWEEP_FWD_PLAIN, SWEEP_FWD_LORA, SWEEP_BWD_1, SWEEP_BWD_2, SWEEP_BWD_PG = 32768, 16384, 16384, 32768, 4096
FP8_SCALE = 48.0          # not a power of two, and |y| > 9.33 saturates: the clamp is part of what is compared


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


def rel_rows(a, b):
    """worst row of |a - b| / |b| (2-norms, fp64); a zero reference row must be met exactly"""
    a, b = a.double(), b.double()
    return ((a - b).norm(dim=1) / (b.norm(dim=1) + 1e-300)).max().item()


def where_for(M, dev):
    return dev if M >= 4096 else torch.device("cpu")


def row_subset(M, sweep, where):
    """>= 4096 rows (all of them below that): the first and last 8, two rows on either side of every sweep boundary, and an even stride"""
    rows = set(range(min(8, M))) | set(range(max(M - 8, 0), M)) | set(range(0, M, max(1, M // 4096)))
    for b in range(sweep, M, sweep):
        rows |= {b - 2, b - 1, b, b + 1}
    rows = sorted(r for r in rows if 0 <= r < M)
    assert len(rows) >= min(M, 4096) and {0, M - 1} <= set(rows)
    return torch.tensor(rows, dtype=torch.int64, device=where)


def nan_buf(dev, dtype, *shape):
    if dtype == FP8:
        return torch.full(shape, 0x7F, dtype=U8, device=dev).view(FP8)        # 0x7f: e4m3's NaN
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def drop_factors(drop_p, seed, M, H, where):
    """0 or 1 / (1 - p) per element, element index row * H + col: the oracle's statement of the kernels' mask"""
    from oracle.clibd_oracle import drop_factor

    idx = torch.arange(M * H, dtype=torch.int64, device=where).view(M, H)
    return drop_factor(seed, idx, drop_p).to(where)


# ------------------------------------------------------------------------------------------------------------------ forward
def fwd_inputs(M, H, seed, where, kind="regular"):
    g = torch.Generator(device=where).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=where)
    x = {"regular": lambda: r(M, H) * 2 + 0.5, "offset": lambda: r(M, H) + 100.0, "outlier": lambda: r(M, H), "tiny": lambda: r(M, H) * 1e-3,
         "const": lambda: r(M, H) * 2 + 0.5}[kind]()
    if kind == "outlier":
        x[:, H - 1] = 300.0
    if kind == "const":
        x[0] = 0.5
        x[1] = 0.0
    return x, r(H), r(H), r(8, H) * 0.05


def fwd_ref(x, gamma, beta, eps):
    xd = x.double()
    y = Fn.layer_norm(xd, (x.shape[1],), gamma.double(), beta.double(), eps)
    return y, xd.mean(1), (xd.var(1, unbiased=False) + eps).rsqrt()


def run_fwd(ops, dev, x, gamma, beta, eps, acat, drop, want):
    """one launch writing exactly the outputs named in `want`, every buffer NaN beforehand"""
    M, H = x.shape
    out = {k: nan_buf(dev, dt, *s) for k, dt, s in (("y_f32", F32, (M, H)), ("y_bf16", BF16, (M, H)), ("y_fp8", FP8, (M, H)), ("stats", F32, (M, 2)))
           if k in want}
    kw = dict(out)
    if acat is not None:
        out["t_out"] = nan_buf(dev, BF16, M, 8)
        kw.update(lora_a=acat.to(dev, BF16), t_out=out["t_out"])
    if "y_fp8" in want:
        kw["fp8_scale"] = FP8_SCALE
    ops.layernorm_fwd(x.to(dev), gamma.to(dev), beta.to(dev), eps, drop=drop, **kw)
    torch.cuda.synchronize()
    return out


def check_fwd(ops, dev, M, H, lora, eps, seed, drop_p=0.0, kind="regular", y_bound=None, mean_bound=None, rstd_bound=1e-5):
    """The full call (y_f32, y_bf16, stats, t_out together) and the three single-output calls against fp64.  Returns the inputs and the full
    call's outputs.  y_bound / mean_bound: per-row bounds as functions of (x, gamma) in place of the regular 2e-5 / 1e-5."""
    where = where_for(M, dev)
    x, gamma, beta, acat = fwd_inputs(M, H, seed, where, kind)
    acat = acat if lora else None
    yref, mean, rstd = fwd_ref(x, gamma, beta, eps)
    drop, fac = None, None
    if drop_p > 0:
        drop = ops.Drop(drop_p, 4242 + seed)
        fac = drop_factors(drop_p, drop.seed, M, H, where)
        yref = yref * fac.double()
    tag = f"M={M} H={H} lora={lora} eps={eps:g} {kind} p={drop_p}"
    y_lim = torch.full((M,), 2e-5, dtype=F64, device=where) if y_bound is None else y_bound(x, gamma)
    mean_lim = torch.full((M,), 1e-5, dtype=F64, device=where) if mean_bound is None else mean_bound(x, gamma)
    full = {k: v.to(where) for k, v in run_fwd(ops, dev, x, gamma, beta, eps, acat, drop, ("y_f32", "y_bf16", "stats")).items()}
    yf = full["y_f32"]
    err = (yf.double() - yref).abs().amax(1)
    assert bool((err < y_lim).all()), (tag, (err / y_lim).max().item())
    if fac is not None:
        assert torch.equal(yf == 0, fac == 0), tag                                     # the zero set is exactly the oracle's
    assert torch.equal(full["y_bf16"], yf.bfloat16()), tag
    merr = (full["stats"][:, 0].double() - mean).abs()
    assert bool((merr < mean_lim).all()), (tag, (merr / mean_lim).max().item())
    rerr = ((full["stats"][:, 1].double() - rstd).abs() / rstd).max().item()
    assert rerr < rstd_bound, (tag, rerr)
    if lora:
        tref = full["y_bf16"].double() @ acat.bfloat16().double().T
        assert (full["t_out"].double() - tref).abs().max().item() < 2e-2 * tref.abs().max().item() + 1e-3, tag
    # single outputs: the buffer asked for is written everywhere (it was NaN), the pointers left NULL are not touched
    one = run_fwd(ops, dev, x, gamma, beta, eps, acat, drop, ("y_f32",))["y_f32"].to(where)
    assert bool(((one.double() - yref).abs().amax(1) < y_lim).all()), tag              # (a NaN left behind fails the comparison)
    one = run_fwd(ops, dev, x, gamma, beta, eps, acat, drop, ("y_bf16",))["y_bf16"].to(where)
    assert torch.equal(one, yf.bfloat16()), tag
    one = run_fwd(ops, dev, x, gamma, beta, eps, acat, drop, ("y_fp8",))["y_fp8"].cpu()
    assert torch.equal(one.view(U8), (yf.cpu() * FP8_SCALE).clamp(-448.0, 448.0).to(FP8).view(U8)), tag
    return x, gamma, beta, full


@pytest.mark.parametrize("M", [1, 3, 6, 37])            # shorter than, equal to (3 / 4 of it) and longer than one wave's 2 or 4 rows
@pytest.mark.parametrize("lora", [False, True], ids=["plain4", "lora2"])
@pytest.mark.parametrize("H", HS)
def test_forward_every_instantiation(ops, dev, H, lora, M):
    """layernorm_fwd_kernel<N, false, 4> and <N, true, 2>, N = 1..4, full and partial last chunks, both towers' eps."""
    for eps in (1e-6, 1e-12):
        check_fwd(ops, dev, M, H, lora, eps, seed=H + M + (1000 if lora else 0))


@pytest.mark.parametrize("H,lora,M", [(64, False, SWEEP_FWD_PLAIN + 5), (768, False, SWEEP_FWD_PLAIN + 5),
                                      (64, True, SWEEP_FWD_LORA + 3), (768, True, SWEEP_FWD_LORA + 3)])
def test_forward_second_sweep_with_a_ragged_tail(ops, dev, H, lora, M):
    """M crosses the grid stride: the last waves take the loop a second time, and the final wave has rows past M.  Every row is judged."""
    check_fwd(ops, dev, M, H, lora, 1e-6 if lora else 1e-12, seed=M + H)


# ------------------------------------------------------------------------------------------------------------------ backward
class Cfg(NamedTuple):
    name: str
    dy: torch.dtype          # bf16 or fp32 upstream gradient
    res: str                 # incoming residual gradient: "none", "f32" (dres) or "bf16" (dres_bf16)
    outs: str                # any of f (dx_f32), b (dx_bf16), r (dx_res_bf16)
    pg: str = "off"          # dgamma / dbeta: "off", "atomic", "ordered"
    fp8: bool = False        # dx_fp8 + row_dequant


CFGS = [
    # B1 (B2 where the two-row condition holds): all seven output subsets
    Cfg("a1", F32, "none", "f"), Cfg("a2", BF16, "f32", "fb"), Cfg("a3", BF16, "bf16", "r"),
    Cfg("a4", F32, "f32", "r"),                        # fp32 dres together with dx_res_bf16: accepted since the unified entry
    Cfg("a5", BF16, "none", "b"), Cfg("a6", F32, "bf16", "fbr"), Cfg("a7", BF16, "bf16", "br"), Cfg("a8", F32, "none", "fr"),
    # PG
    Cfg("c1", F32, "f32", "f", pg="atomic"), Cfg("c2", BF16, "bf16", "br", pg="ordered"), Cfg("c3", BF16, "none", "fb", pg="ordered"),
    Cfg("c4", F32, "f32", "r", pg="atomic"),
    # F8-1 (F8-2 where the two-row condition holds)
    Cfg("d1", BF16, "bf16", "r", fp8=True), Cfg("d2", F32, "f32", "fr", fp8=True), Cfg("d3", BF16, "bf16", "br", fp8=True),
    Cfg("d4", BF16, "none", "", fp8=True),              # the e4m3 rows as the only output
    # F8-PG
    Cfg("e1", BF16, "bf16", "br", pg="atomic", fp8=True), Cfg("e2", F32, "f32", "f", pg="ordered", fp8=True),
    Cfg("e3", BF16, "none", "b", pg="ordered", fp8=True),
]
CFG = {c.name: c for c in CFGS}


def bwd_inputs(M, H, seed, where, kind="regular"):
    """dy and the residual gradient carry one power-of-two scale per row (2^-20 .. 2^3): every exponent path of the e4m3 row scale; row 3 is zero"""
    g = torch.Generator(device=where).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=where)
    x = fwd_inputs(M, H, seed + 1, where, kind)[0]
    sc = torch.exp2(torch.randint(-20, 4, (M, 1), generator=g, device=where).float())
    d = dict(x=x, gamma=r(H), beta=r(H), dy=r(M, H) * sc, dres=r(M, H) * sc, dg0=r(H), db0=r(H))
    if M > 3:
        d["dy"][3] = 0
        d["dres"][3] = 0
    return d


def bwd_ref(d, cfg, eps, rows=None, want_pg=False):
    """fp64 autograd of layer_norm (+ the residual): dx on `rows`, the column sums over all rows; (mean, rstd) of all rows as fp32"""
    H = d["x"].shape[1]
    xd_all = d["x"].double()
    stats = torch.stack([xd_all.mean(1), (xd_all.var(1, unbiased=False) + eps).rsqrt()], dim=1).float().contiguous()
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    xd = sel(d["x"]).double().requires_grad_(True)
    gd, bd = d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    dy = sel(d["dy"]) if cfg.dy == F32 else sel(d["dy"]).bfloat16()
    dx, dg, db = torch.autograd.grad(Fn.layer_norm(xd, (H,), gd, bd, eps), (xd, gd, bd), dy.double())
    if cfg.res == "f32":
        dx = dx + sel(d["dres"]).double()
    elif cfg.res == "bf16":
        dx = dx + sel(d["dres"]).bfloat16().double()
    assert rows is None or not want_pg
    return dx, d["dg0"].double() + dg, d["db0"].double() + db, stats


def run_bwd(ops, dev, d, cfg, stats, drop=None, extra_f32=False):
    M, H = d["x"].shape
    outs = cfg.outs + ("f" if extra_f32 and "f" not in cfg.outs else "")
    o = {}
    kw = {}
    for key, name, dt in (("f", "dx_f32", F32), ("b", "dx_bf16", BF16), ("r", "dx_res_bf16", BF16)):
        if key in outs:
            o[name] = kw[name] = nan_buf(dev, dt, M, H)
    if cfg.fp8:
        o["dx_fp8"], o["row_dequant"] = nan_buf(dev, FP8, M, H), nan_buf(dev, F32, M)
        kw.update(dx_fp8=o["dx_fp8"], row_dequant=o["row_dequant"])
    if cfg.pg != "off":
        o["dgamma"], o["dbeta"] = d["dg0"].to(dev).clone(), d["db0"].to(dev).clone()      # non-zero contents: the kernel accumulates
        kw.update(dgamma=o["dgamma"], dbeta=o["dbeta"], ordered=cfg.pg == "ordered")
    if cfg.res == "f32":
        kw["dres"] = d["dres"].to(dev)
    elif cfg.res == "bf16":
        kw["dres_bf16"] = d["dres"].to(dev, BF16)
    ops.layernorm_bwd(d["dy"].to(dev, cfg.dy), d["x"].to(dev), stats.to(dev), d["gamma"].to(dev), drop=drop, **kw)
    torch.cuda.synchronize()
    return o


def e4m3_half_step(w):
    """half the spacing of e4m3 at |w| (three mantissa bits; subnormals below 2^-6 are spaced 2^-9)"""
    return 0.5 * torch.exp2(torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -6))) - 3.0)


def check_fp8_rows(d8, rd, ref, tag):
    """dequantised e4m3 rows against the fp64 value: each element within half an e4m3 step at its own magnitude under the row's scale (never
    more than the 8 of the top binade), plus the fp32 error the value itself is allowed (2e-5 of the row maximum, < 256 after scaling).
    The reference's row maximum, scaled by the kernel's power-of-two scale, must lie in [128, 256); a zero row takes scale 1."""
    rd = rd.double()
    assert bool(((torch.log2(rd) % 1.0) == 0).all()) and bool((rd > 0).all()), tag      # powers of two
    w = ref / rd[:, None]
    amax = w.abs().amax(1)
    live = ref.abs().amax(1) > 0
    assert bool((amax[live] >= 128.0).all()) and bool((amax[live] < 256.0).all()), (tag, amax[live].min().item(), amax[live].max().item())
    assert bool((rd[~live] == 1.0).all()) and int(d8.view(U8)[~live].max() if (~live).any() else 0) == 0, tag
    err = (d8.double() - w).abs()
    assert bool((err <= e4m3_half_step(w) + 2e-5 * 256.0).all()), (tag, (err - e4m3_half_step(w)).max().item())


def check_bwd(ops, dev, M, H, cfg, seed, eps=1e-6, rows=None, drop_p=0.0, kind="regular", two_row=False, dx_bound=2e-5):
    where = where_for(M, dev)
    d = bwd_inputs(M, H, seed, where, kind)
    ref, dg_ref, db_ref, stats = bwd_ref(d, cfg, eps, rows, want_pg=cfg.pg != "off")
    sel = (lambda t: t.to(where)) if rows is None else (lambda t: t[rows.to(t.device)].to(where))
    drop, fac = None, torch.ones((), device=where)
    if drop_p > 0:
        drop = ops.Drop(drop_p, 777 + seed)
        fac = sel(drop_factors(drop_p, drop.seed, M, H, where))
    tag = f"{cfg.name} M={M} H={H} {kind} p={drop_p}"
    o = run_bwd(ops, dev, d, cfg, stats, drop)
    if two_row:
        # dx_f32 would select the one-row kernel: the bf16 outputs themselves against bf16(fp64), at the project's bf16 bound
        assert "f" not in cfg.outs and cfg.dy == BF16 and cfg.res != "f32" and cfg.pg == "off" and M >= 131072
        for name, f in (("dx_res_bf16", 1.0), ("dx_bf16", fac)):
            if name in o:
                assert rel_rows(sel(o[name]).float(), (ref * f).bfloat16().float()) < 4e-3, (tag, name)
    else:
        val = o["dx_f32"] if "f" in cfg.outs else run_bwd(ops, dev, d, cfg, stats, drop, extra_f32=True)["dx_f32"]
        val = sel(val)
        assert bool(torch.isfinite(val).all()), tag
        assert rel_rows(val, ref) < dx_bound, (tag, rel_rows(val, ref))                # dx_f32 never carries the mask
        if "dx_res_bf16" in o:
            assert torch.equal(sel(o["dx_res_bf16"]), val.bfloat16()), tag             # nor does the residual copy
        if "dx_bf16" in o:
            assert torch.equal(sel(o["dx_bf16"]), (val * fac).bfloat16()), tag         # the dense branch's copy does
            if drop_p > 0:
                assert torch.equal(sel(o["dx_bf16"])[val != 0] == 0, (fac == 0)[val != 0]), tag
    if cfg.fp8:
        d8 = sel(o["dx_fp8"].view(U8)).view(FP8)
        check_fp8_rows(d8, sel(o["row_dequant"]), ref * fac, tag)
        if drop_p > 0:                                                                 # the e4m3 copy carries the mask
            assert int((d8.view(U8)[fac == 0] & 0x7F).max()) == 0, tag                 # (a dropped negative value is -0: the sign bit alone)
            assert float((d8.float()[fac != 0] != 0).float().mean()) > 0.9, tag
    if cfg.pg != "off":
        for name, want in (("dgamma", dg_ref), ("dbeta", db_ref)):
            got = o[name].to(where).double()
            assert ((got - want).norm() / want.norm()).item() < 2e-4, (tag, name)
        if cfg.pg == "ordered":
            again = run_bwd(ops, dev, d, cfg, stats, drop)
            assert torch.equal(again["dgamma"], o["dgamma"]) and torch.equal(again["dbeta"], o["dbeta"]), tag
    return o


@pytest.mark.parametrize("cfg", CFGS, ids=[c.name for c in CFGS])
@pytest.mark.parametrize("H", HS)
def test_backward_every_form_small(ops, dev, H, cfg):
    """M = 1, 2, 5, 37 through every operand set: B1 (a*), PG (c*), F8-1 (d*), F8-PG (e*), N = 1..4."""
    for M in (1, 2, 5, 37):
        check_bwd(ops, dev, M, H, cfg, seed=H * 7 + M)


@pytest.mark.parametrize("name", ["a2", "a7", "d1", "d2"])
@pytest.mark.parametrize("H", [128, 768])
def test_backward_one_row_second_sweep(ops, dev, H, name):
    """M = 16384 + 1: one wave of the one-row kernels (B1, F8-1) walks the grid stride a second time."""
    check_bwd(ops, dev, SWEEP_BWD_1 + 1, H, CFG[name], seed=H + 11)


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c4", "e1", "e2", "e3"])
@pytest.mark.parametrize("H", [128, 768])
def test_backward_parameter_gradients_second_sweep(ops, dev, H, name):
    """M = 4096 + 3 crosses the parameter-gradient grid (1024 blocks): PG and F8-PG, atomic and ordered, against fp64 column sums."""
    check_bwd(ops, dev, SWEEP_BWD_PG + 3, H, CFG[name], seed=H + 13)


@pytest.mark.parametrize("H,name", [(128, "a5"), (128, "a7"), (128, "d1"), (128, "d3"), (768, "a7"), (768, "d1")])
def test_backward_two_row_forms(ops, dev, H, name):
    """M = 131072 + 3: B2 (a5, a7) and F8-2 (d1, d3); four sweeps of 32768 rows and a last wave whose second row is past M."""
    M = 131072 + 3
    check_bwd(ops, dev, M, H, CFG[name], seed=H + 17, rows=row_subset(M, SWEEP_BWD_2, dev), two_row=True)


def test_backward_fp8_four_chunks_falls_back_to_one_row(ops, dev):
    """M = 131072 + 3 with N = 4 (H = 832) and dx_fp8: the two-row e4m3 kernel exists up to N = 3, the host must take F8-1."""
    M = 131072 + 3
    check_bwd(ops, dev, M, 832, CFG["d1"], seed=19, rows=row_subset(M, SWEEP_BWD_1, dev), two_row=True)


# ------------------------------------------------------------------------------------------------------------------ dropout positions
@pytest.mark.parametrize("M", [37, SWEEP_FWD_LORA + 3])
@pytest.mark.parametrize("lora", [False, True], ids=["plain4", "lora2"])
@pytest.mark.parametrize("H", [64, 768])
def test_dropout_forward_positions(ops, dev, H, lora, M):
    """y = LN(x) * drop_factor(seed, row * H + col, p): values at the regular tolerance, the zero set exactly the oracle's."""
    check_fwd(ops, dev, M, H, lora, 1e-12, seed=M + H + 1, drop_p=0.1)


@pytest.mark.parametrize("M", [37, SWEEP_BWD_1 + 3])
@pytest.mark.parametrize("cfg", [Cfg("drop-B1", BF16, "bf16", "fbr"), Cfg("drop-F8-1", BF16, "bf16", "fbr", fp8=True),
                                 Cfg("drop-PG", F32, "f32", "fbr", pg="atomic"), Cfg("drop-F8-PG", BF16, "none", "br", pg="ordered", fp8=True)],
                         ids=lambda c: c.name)
@pytest.mark.parametrize("H", [64, 768])
def test_dropout_backward_positions(ops, dev, H, cfg, M):
    """dx_bf16 and the e4m3 rows carry the mask of element row * H + col, dx_f32 and dx_res_bf16 do not."""
    check_bwd(ops, dev, M, H, cfg, seed=M + H + 2, drop_p=0.1)


# ------------------------------------------------------------------------------------------------------------------ ill-conditioned inputs
def _offset_y_bound(x, gamma):
    """per row 4 * 2^-23 * (max|x| / sigma) * max|gamma| + 2e-6: the rounding of x - mean at the magnitude of x, carried through rstd and gamma
    (an fp32 restatement of the two-pass arithmetic stayed within 1.4 of that unit; the factor 4 leaves room for the device's rsqrt)"""
    xd = x.double()
    return 4.0 * 2.0 ** -23 * (xd.abs().amax(1) / xd.var(1, unbiased=False).sqrt()) * gamma.abs().max().item() + 2e-6


def _offset_mean_bound(x, gamma):
    """the mean is a sum at the magnitude of x: the same four units of 2^-23 * max|x| that the bound on y grants x - mean"""
    return 4.0 * 2.0 ** -23 * x.double().abs().amax(1) + 1e-30


# an fp32 CPU restatement of the backward (stats from fp64 as here) measured at most 1.61e-6 per row against fp64 on these two inputs
# (H in {64, 320, 768, 1024}, both eps, 20 seeds each); the kernel is allowed 5 x that
OFFSET_DX_BOUND = 5 * 1.61e-6


@pytest.mark.parametrize("kind", ["offset", "outlier"])
@pytest.mark.parametrize("eps", [1e-6, 1e-12])
@pytest.mark.parametrize("lora", [False, True], ids=["plain4", "lora2"])
@pytest.mark.parametrize("H", [64, 768])
def test_large_mean_against_small_spread(ops, dev, H, lora, eps, kind):
    """x = randn + 100 (|mean| / sigma = 100) and one channel at 300: a one-pass variance is off by >= 1e-4 in rstd, the two-pass one by 1e-7."""
    check_fwd(ops, dev, 8, H, lora, eps, seed=H + 23, kind=kind, y_bound=_offset_y_bound, mean_bound=_offset_mean_bound, rstd_bound=1e-6)
    for name in ("a1", "a2", "c1"):
        check_bwd(ops, dev, 8, H, CFG[name], seed=H + 29, eps=eps, kind=kind, dx_bound=OFFSET_DX_BOUND)


@pytest.mark.parametrize("eps", [1e-6, 1e-12])
@pytest.mark.parametrize("lora", [False, True], ids=["plain4", "lora2"])
@pytest.mark.parametrize("H", [64, 768])
def test_constant_and_zero_rows(ops, dev, H, lora, eps):
    """Row 0 is the constant 0.5, row 1 is zero: the mean is exact, y is beta bit for bit, and the backward at xhat = 0 is finite and the fp64 value."""
    x, gamma, beta, full = check_fwd(ops, dev, 8, H, lora, eps, seed=H + 31, kind="const")
    assert full["stats"][0, 0].item() == 0.5 and full["stats"][1, 0].item() == 0.0
    assert torch.equal(full["y_f32"][0], beta) and torch.equal(full["y_f32"][1], beta)
    for name in ("a1", "a7", "c3", "d2"):
        check_bwd(ops, dev, 8, H, CFG[name], seed=H + 30, eps=eps, kind="const")


@pytest.mark.parametrize("lora", [False, True], ids=["plain4", "lora2"])
@pytest.mark.parametrize("H", [64, 768])
def test_tiny_activations_at_the_bert_eps(ops, dev, H, lora):
    """x = randn * 1e-3 with eps = 1e-12 (var = 1e-6): the regular tolerances."""
    check_fwd(ops, dev, 8, H, lora, 1e-12, seed=H + 37, kind="tiny")
    for name in ("a1", "a6", "c1", "d2"):
        check_bwd(ops, dev, 8, H, CFG[name], seed=H + 36, eps=1e-12, kind="tiny")


@pytest.mark.parametrize("name", ["d4", "d3", "e1"])
@pytest.mark.parametrize("H", [64, 768])
def test_zero_gradient_rows_quantise_to_scale_one(ops, dev, H, name):
    """dy = 0 (and a zero residual): row_dequant is 1 and every e4m3 byte is zero, never a NaN from a zero maximum."""
    M, cfg = 8, CFG[name]
    d = bwd_inputs(M, H, H + 41, torch.device("cpu"))
    d["dy"].zero_()
    d["dres"].zero_()
    stats = bwd_ref(d, cfg, 1e-12)[3]
    o = run_bwd(ops, dev, d, cfg, stats)
    assert torch.equal(o["row_dequant"].cpu(), torch.ones(M)) and int(o["dx_fp8"].view(U8).max()) == 0
    for k in ("dx_bf16", "dx_res_bf16"):
        if k in o:
            assert int((o[k].float() != 0).sum()) == 0
