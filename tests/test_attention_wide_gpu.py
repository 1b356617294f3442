"""The 128- and 192-wide attention kernels (csrc/attention_wide.hip) against an fp64 statement of the operation (GPU).

Dispatch of clibd_attention_wide_fwd / clibd_attention_wide_bwd, read from the host code: N = 2 * ceil(S / 32) key tiles of 16 (S 1..32 -> 2, ...,
225..256 -> 16; at head_dim 192 S <= 192, N <= 12), DROP = drop_thr16 > 0; one instantiation <head_dim, N, DROP> per kernel, one workgroup per
(sequence, head); the forward runs four waves at N <= 4 (S = 1 .. 33 below) and eight at N >= 6 (every other S), the backward always four.  The cases below take every N on both sides of its edges (S = 16 | 17, 32 | 33, 160 | 161, 192 | 193, 255 | 256), the all-padding
last tile (S = 133: 9 live tiles of 10; S = 161: 11 of 12), a single key (S = 1) and both widths' largest S.

The method is that of tests/test_attention_forms_gpu.py with a head-width parameter.  Reference: softmax(q k^T / sqrt(head_dim)) in fp64 times the
oracle's dropout factor for element ((b * nh + h) * S + q) << 8 | key (oracle.clibd_oracle.drop_factor), times v; gradients by torch autograd in fp64.

Judgement, per (sequence, head): the 2-norm of the error of every head_dim-element row of out / dq / dk / dv over max(|ref row|, 0.25 * mean row norm
of that (sequence, head)); the worst row must meet the bound.  A (sequence, head) whose reference dq / dk is entirely zero (S = 1: dS = P o (dP -
delta) cancels exactly) is divided by the magnitude of what cancels, sum_k P (|dP| + |delta|) |k_k| scale (|q_q| for dk); any other all-zero reference
(dO = 0) must be met exactly.  Every output sits NaN-filled between sentinel rows that must stay intact.

Bounds: `restate` is the operation in fp32 torch with the kernels' rounding points (un-normalised exp2(c2 s - c2 max) times the drop factor rounded
to bf16 before @ v, the fp32 row sum dividing the fp32 result, out to bf16; backward: normalised P in fp32, dP = (dO V^T) o F, delta = sum(P o dP),
dS to bf16 before both products, P o F to bf16 before dV, outputs to bf16).  `python tests/test_attention_wide_gpu.py` runs it on the CPU over
every host-made input of this module (and host-drawn operands of the many-workgroup shape) and prints the worst floored row errors per head width:
    head_dim 128: forward 4.309e-03 (one-hot v, S = 133, keys 128 .. 132: rows of five non-zero elements)   backward 4.381e-03 (dk, S = 224, randn)
                  lse 2.471e-05 (absolute, log2 domain: S = 133, operands x 4, where |lse| is in the hundreds)
    head_dim 192: forward 3.249e-03 (the many-workgroup shape, S = 133, p = 0.1)   backward 4.266e-03 (dk, S = 192, operands x 4)
                  lse 2.702e-05 (S = 192, operands x 4)
FWD_BOUND / BWD_BOUND are 3 x those per width (the kernels' v_exp / v_log / reciprocal, the MFMA accumulation order and P from the saved lse live in
the margin; one misplaced element in a row of 128 is an error near 0.12), LSE_BOUND 4 x, never above the project's 2e-3.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
CPU = torch.device("cpu")
PAD = 3                       # sentinel rows (elements for lse) in front of and behind every output
P_DROP = 0.1
B0, NH0 = 2, 2                # the host-made cases
DHS = (128, 192)
MAX_S = {128: 256, 192: 192}
WORST = {128: dict(fwd=4.309e-3, bwd=4.381e-3, lse=2.471e-5), 192: dict(fwd=3.249e-3, bwd=4.266e-3, lse=2.702e-5)}   # measured on the CPU: see the docstring
FWD_BOUND = {dh: 3 * w["fwd"] for dh, w in WORST.items()}
BWD_BOUND = {dh: 3 * w["bwd"] for dh, w in WORST.items()}
LSE_BOUND = {dh: min(4 * w["lse"], 2e-3) for dh, w in WORST.items()}


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ------------------------------------------------------------------------------------------------------------------ operands
KINDS = ["randn", "x4", "bigrow", "do0", "half"]


@functools.lru_cache(maxsize=None)
def inputs(dh, B, S, nh, kind="randn"):
    """(qkv [B*S, 3H], dO [B*S, H]) as bf16 on the host, made once per shape and never modified"""
    g = torch.Generator().manual_seed(1000000 * KINDS.index(kind) + 1000 * S + 10 * B + nh + 7 * dh)
    H = dh * nh
    qkv, do = torch.randn(B * S, 3 * H, generator=g), torch.randn(B * S, H, generator=g)
    if kind == "x4":
        qkv *= 4.0
    elif kind == "half":
        qkv *= 0.5
    elif kind == "bigrow":                      # one query row 30 times larger: sequence 0 in the middle, sequence 1 the last (the clamped) row
        x = qkv.view(B, S, 3 * H)
        x[0, S // 2, :H] *= 30.0
        x[1, S - 1, :H] *= 30.0
    elif kind == "do0":
        do.zero_()
    return qkv.bfloat16(), do.bfloat16()


def split(qkv, B, S, nh, dh):
    """[B*S, 3H] -> q, k, v each [B, nh, S, dh]"""
    return qkv.view(B, S, 3, nh, dh).permute(2, 0, 3, 1, 4)


def heads(t, B, n, nh, dh):
    """[B*n, H] -> [B, nh, n, dh]"""
    return t.view(B, n, nh, dh).permute(0, 2, 1, 3)


def drop_fac(p, seed, seqs, nh, S, where):
    """the oracle's 0 or 1 / (1 - p) for element ((b * nh + h) * S + q) << 8 | key of the (global) sequences `seqs`: [len(seqs), nh, S, S]"""
    from oracle.clibd_oracle import drop_factor

    b = torch.as_tensor(list(seqs), dtype=torch.int64, device=where).view(-1, 1, 1, 1)
    h = torch.arange(nh, dtype=torch.int64, device=where).view(1, nh, 1, 1)
    q = torch.arange(S, dtype=torch.int64, device=where).view(1, 1, S, 1)
    key = torch.arange(S, dtype=torch.int64, device=where).view(1, 1, 1, S)
    return drop_factor(seed, (((b * nh + h) * S + q) << 8) | key, p).to(where)


# ------------------------------------------------------------------------------------------------------------------ the two statements
def reference(qkv, do, B, S, nh, dh, fac, grad=True):
    """fp64: out [B, nh, S, dh], lse (log2 domain) [B, nh, S], and dq, dk, dv [B, nh, S, dh] by autograd.  Plain: no rounding anywhere."""
    scale = 1.0 / math.sqrt(dh)
    x = qkv.double().requires_grad_(grad)
    q, k, v = split(x, B, S, nh, dh)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    if fac is not None:
        p = p * fac.double()
    o = p @ v
    r = dict(o=o.detach(), lse=(torch.logsumexp(s, dim=-1) * LOG2E).detach())
    if grad:
        doh = heads(do.double(), B, S, nh, dh)
        (gx,) = torch.autograd.grad(o, x, doh)
        r["dq"], r["dk"], r["dv"] = split(gx, B, S, nh, dh)
        with torch.no_grad():       # what cancels in dS = P o (dP - delta): the scale of dq / dk rows where the statement itself is exactly zero
            pd = torch.softmax(s, dim=-1)
            dp = doh @ v.transpose(-1, -2) * (1.0 if fac is None else fac.double())
            w = pd * (dp.abs() + (pd * dp).sum(-1, keepdim=True).abs())
            r["mag_dq"] = scale * (w @ k.norm(dim=-1, keepdim=True)).squeeze(-1)
            r["mag_dk"] = scale * (w.transpose(-1, -2) @ q.norm(dim=-1, keepdim=True)).squeeze(-1)
    return r


def bfr(t):
    return t.bfloat16().float()


def restate(qkv, do, B, S, nh, dh, fac, grad=True):
    """fp32 with the kernels' rounding points (see the docstring); same results layout as `reference`.  Only used to derive the bounds."""
    scale = torch.tensor(1.0 / math.sqrt(dh), dtype=F32)
    c2 = scale * torch.tensor(LOG2E, dtype=F32)
    q, k, v = split(qkv.float(), B, S, nh, dh)
    s = q @ k.transpose(-1, -2)
    mc = s.amax(-1, keepdim=True) * c2
    e = torch.exp2(s * c2 - mc)
    tot = e.sum(-1, keepdim=True)
    f = torch.ones((), dtype=F32) if fac is None else fac.float()
    r = dict(o=bfr((bfr(e * f) @ v) / tot), lse=(mc + torch.log2(tot)).squeeze(-1))
    if grad:
        doh = heads(do.float(), B, S, nh, dh)
        p = e / tot
        dp = (doh @ v.transpose(-1, -2)) * f
        ds = bfr(p * (dp - (p * dp).sum(-1, keepdim=True)))
        r["dq"] = bfr((ds @ k) * scale)
        r["dk"] = bfr((ds.transpose(-1, -2) @ q) * scale)
        r["dv"] = bfr(bfr(p * f).transpose(-1, -2) @ doh)
    return r


def row_err(got, ref, zero_floor=None):
    """worst head_dim-element row of |got - ref| / max(|ref row|, 0.25 * mean row norm of its (sequence, head)); inputs [..., rows, dh].
    zero_floor [..., rows]: the denominator of a (sequence, head) whose reference is entirely zero; without one it must be met exactly."""
    got, ref = got.double(), ref.double()
    n = ref.norm(dim=-1)
    den = torch.maximum(n, 0.25 * n.mean(dim=-1, keepdim=True))
    if zero_floor is not None:
        den = torch.where(n.amax(dim=-1, keepdim=True) == 0, zero_floor.double(), den)
    den = den.clamp_min(1e-300)
    e = (got - ref).norm(dim=-1) / den
    return e.max().item() if e.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------ launches
def guarded(dev, dtype, rows, *cols):
    """(buffer, view): `rows` NaN rows between PAD sentinel rows on either side"""
    buf = torch.full((rows + 2 * PAD, *cols), float("nan"), dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + rows]


def sentinels_intact(buf):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


def run_fwd(ops, dev, qkv, B, S, nh, dh, drop=None, save=True):
    """one forward launch into NaN-filled, sentinel-guarded buffers"""
    bo, out = guarded(dev, BF16, B * S, nh * dh)
    bl, lse = guarded(dev, F32, B * nh * S)
    ops.attention_wide_fwd(qkv.to(dev), B, S, nh, dh, out, lse=lse if save else None, drop=drop)
    torch.cuda.synchronize()
    assert sentinels_intact(bo) and sentinels_intact(bl), "forward wrote outside its buffers"
    assert bool(torch.isfinite(out.float()).all()), "forward left output rows unwritten (or not finite)"
    if save:
        assert bool(torch.isfinite(lse).all()), "forward left lse unwritten"
    else:
        assert bool(torch.isnan(lse).all()), "forward wrote an lse it was not given"
    return dict(out=out, lse=lse if save else None)


def run_bwd(ops, dev, qkv, do, lse, B, S, nh, dh, drop=None):
    buf, dqkv = guarded(dev, BF16, B * S, 3 * nh * dh)
    ops.attention_wide_bwd(qkv.to(dev), do.to(dev), lse, B, S, nh, dh, dqkv, drop=drop)
    torch.cuda.synchronize()
    assert sentinels_intact(buf), "backward wrote outside dqkv"
    assert bool(torch.isfinite(dqkv.float()).all()), "backward left rows unwritten (or not finite)"
    return dqkv


# ------------------------------------------------------------------------------------------------------------------ host-evaluated cases
@functools.lru_cache(maxsize=None)
def case_data(dh, S, kind, p, seed):
    """operands, drop factors and the fp64 reference of one host case, made once (the CPU measurement takes the same)"""
    qkv, do = inputs(dh, B0, S, NH0, kind)
    fac = drop_fac(p, seed & 0xFFFFFFFF, range(B0), NH0, S, CPU) if p > 0 else None
    return qkv, do, fac, reference(qkv, do, B0, S, NH0, dh, fac)


def judge(got, ref, dh, tag):
    e = row_err(got["o"], ref["o"])
    print(f"{tag}: out {e:.3e}", end="")
    assert e < FWD_BOUND[dh], (tag, "out", e)
    if "lse" in got:
        e = (got["lse"].double() - ref["lse"]).abs().max().item()
        print(f" lse {e:.3e}", end="")
        assert e < LSE_BOUND[dh], (tag, "lse", e)
    for name in ("dq", "dk", "dv"):
        if name in got:
            e = row_err(got[name], ref[name], ref["mag_" + name] if name != "dv" else None)
            print(f" {name} {e:.3e}", end="")
            assert e < BWD_BOUND[dh], (tag, name, e)
    print()


def check(ops, dev, dh, S, kind="randn", p=0.0):
    """forward and backward of one host case against fp64, per row; the same launches a second time give the same bits"""
    seed = 4242 + S
    qkv, do, fac, ref = case_data(dh, S, kind, p, seed)
    drop = ops.Drop(p, seed) if p > 0 else None
    tag = f"dh={dh} S={S} {kind} p={p}"
    fw = run_fwd(ops, dev, qkv, B0, S, NH0, dh, drop)
    plain = run_fwd(ops, dev, qkv, B0, S, NH0, dh, drop, save=False)
    assert torch.equal(plain["out"], fw["out"]), (tag, "the lse-saving forward changes out")
    dqkv = run_bwd(ops, dev, qkv, do, fw["lse"], B0, S, NH0, dh, drop)
    dq, dk, dv = split(dqkv.cpu().float(), B0, S, NH0, dh)
    got = dict(o=heads(fw["out"].cpu().float(), B0, S, NH0, dh), lse=fw["lse"].cpu().view(B0, NH0, S), dq=dq, dk=dk, dv=dv)
    judge(got, ref, dh, tag)
    fw2 = run_fwd(ops, dev, qkv, B0, S, NH0, dh, drop)
    assert torch.equal(fw2["out"], fw["out"]) and torch.equal(fw2["lse"], fw["lse"]), (tag, "forward not reproducible")
    assert torch.equal(run_bwd(ops, dev, qkv, do, fw["lse"], B0, S, NH0, dh, drop), dqkv), (tag, "backward not reproducible")
    return got, ref


S_BOTH = [1, 16, 17, 32, 33, 133, 160, 161, 192]
S_128 = [193, 224, 255, 256]
CASES_S = [(dh, S, p) for dh in DHS for S in S_BOTH + (S_128 if dh == 128 else []) for p in (0.0, P_DROP)]
CASES_KIND = [(dh, kind, S) for dh in DHS for kind in ("randn", "x4", "bigrow", "do0") for S in (133, MAX_S[dh])]
CASES_POS = [(dh, S) for dh in DHS for S in (133, MAX_S[dh])]
MANY_S = 133


def host_cases():
    """every (dh, S, kind, p, seed) the host-evaluated tests use: the inputs the bounds are measured on"""
    for dh, S, p in CASES_S:
        yield dh, S, "randn", p, 4242 + S
    for dh, kind, S in CASES_KIND:
        yield dh, S, kind, 0.0, 4242 + S


@pytest.mark.parametrize("dh,S,p", CASES_S, ids=[f"dh{dh}-S{S}-p{p}" for dh, S, p in CASES_S])
def test_every_tile_count(ops, dev, dh, S, p):
    """every key-tile count of both widths on both sides of its edges, with and without dropout; S = 1 is a single key (the statement's dq and dk are
    exactly zero: judged against the magnitude of what cancels)"""
    got, ref = check(ops, dev, dh, S, p=p)
    if S == 1:
        assert float(ref["dq"].abs().max()) == 0.0 and float(ref["dk"].abs().max()) == 0.0


@pytest.mark.parametrize("dh,kind,S", CASES_KIND, ids=[f"dh{dh}-{k}-S{S}" for dh, k, S in CASES_KIND])
def test_value_edges(ops, dev, dh, kind, S):
    """peaked softmax (x 4), one query row 30 times larger than the rest (once the last, clamped row), dO = 0 (dqkv exactly zero)"""
    got, ref = check(ops, dev, dh, S, kind=kind)
    if kind == "do0":
        assert all(float(got[n].abs().max()) == 0.0 for n in ("dq", "dk", "dv"))


# ---- dropout positions, exactly
def one_hot_v(qkv, B, S, nh, dh, c):
    """v of key dh c + d is the unit vector e_d (every other key's v is zero): out[q, d] reads P[q, dh c + d] * F[q, dh c + d] back"""
    x = qkv.clone().view(B, S, 3, nh, dh)
    x[:, :, 2] = 0
    w = min(dh, S - dh * c)
    d = torch.arange(w, device=qkv.device)
    x[:, dh * c + d, 2, :, d] = 1.0
    return x.view(B * S, 3 * dh * nh), w


def check_positions(out, fac, ref, dh, c, w, tag):
    """out [B, nh, S, dh] (fp32), fac [B, nh, S, S]: the zero set of columns 0 .. w-1 is exactly the oracle's dropped set of keys dh c .. dh c + w - 1,
    the columns without a key are zero, and the values meet the forward bound"""
    gone = fac[..., dh * c:dh * c + w] == 0
    assert torch.equal(out[..., :w] == 0, gone), (tag, c, int(((out[..., :w] == 0) != gone).sum()))
    assert bool((out[..., w:] == 0).all()), (tag, c)
    assert 0.03 < float(gone.double().mean()) < 0.2, tag              # the mask is a mask of p = 0.1
    e = row_err(out, ref["o"])
    assert e < FWD_BOUND[dh], (tag, c, e)


@pytest.mark.parametrize("dh,S", CASES_POS, ids=[f"dh{dh}-S{S}" for dh, S in CASES_POS])
def test_dropout_positions_forward(ops, dev, dh, S):
    """which probabilities are dropped, element by element, against the oracle's hash of ((head * S + q) << 8) | key (a seed whose high bit is set)"""
    seed = 0x9E3779B1
    qkv, _ = inputs(dh, B0, S, NH0, "half")
    drop = ops.Drop(P_DROP, seed)
    fac = drop_fac(P_DROP, drop.seed, range(B0), NH0, S, CPU)
    for c in range((S + dh - 1) // dh):
        x, w = one_hot_v(qkv, B0, S, NH0, dh, c)
        ref = reference(x, None, B0, S, NH0, dh, fac, grad=False)
        out = heads(run_fwd(ops, dev, x, B0, S, NH0, dh, drop)["out"].cpu().float(), B0, S, NH0, dh)
        check_positions(out, fac, ref, dh, c, w, f"dh={dh} S={S}")


@pytest.mark.parametrize("dh,S", CASES_POS, ids=[f"dh{dh}-S{S}" for dh, S in CASES_POS])
def test_dropout_positions_backward(ops, dev, dh, S):
    """the dK / dV phase indexes the mask one key per lane (the dQ phase four keys per lane, as the forward: held by the bounds above): with
    dO = e_0 in ONE query row and zero elsewhere, dV[key, 0] = (P o F)[that query, key], so the zero set of dV[:, 0] is that query's dropped set"""
    seed = 0x9E3779B1
    qkv, _ = inputs(dh, B0, S, NH0, "half")
    drop = ops.Drop(P_DROP, seed)
    fac = drop_fac(P_DROP, drop.seed, range(B0), NH0, S, CPU)
    fw = run_fwd(ops, dev, qkv, B0, S, NH0, dh, drop)
    for qrow in sorted({0, S // 2, S - 1}):
        do = torch.zeros(B0, S, NH0, dh)
        do[:, qrow, :, 0] = 1.0
        dqkv = run_bwd(ops, dev, qkv, do.view(B0 * S, NH0 * dh).bfloat16(), fw["lse"], B0, S, NH0, dh, drop)
        dv = split(dqkv.cpu().float(), B0, S, NH0, dh)[2]
        assert torch.equal(dv[..., 0] == 0, fac[:, :, qrow, :] == 0), (dh, S, qrow)
        assert bool((dv[..., 1:] == 0).all())


# ---- many workgroups
def sample_pairs(B):
    return sorted({0, B // 2, B - 1})


@pytest.mark.parametrize("dh", DHS)
def test_many_workgroups(ops, dev, cus, dh):
    """B * nheads >= 2 x the compute units (operands drawn on the device, dropout on: the element index follows the workgroup); fp64 on a sample of
    sequences, every head of each"""
    nh, S = 2, MANY_S
    B = cus + 1
    assert B * nh >= 2 * cus
    g = torch.Generator(device=dev).manual_seed(dh + S)
    qkv = torch.randn(B * S, 3 * dh * nh, generator=g, device=dev).bfloat16()
    do = torch.randn(B * S, dh * nh, generator=g, device=dev).bfloat16()
    drop = ops.Drop(P_DROP, 1234 + dh)
    fw = run_fwd(ops, dev, qkv, B, S, nh, dh, drop)
    dqkv = run_bwd(ops, dev, qkv, do, fw["lse"], B, S, nh, dh, drop)
    seqs = sample_pairs(B)
    n, sel = len(seqs), torch.as_tensor(seqs, device=dev)
    pick = lambda t: t.view(B, S, -1)[sel].reshape(n * S, -1)
    fac = drop_fac(P_DROP, drop.seed, seqs, nh, S, dev)
    ref = reference(pick(qkv), pick(do), n, S, nh, dh, fac)
    dq, dk, dv = split(pick(dqkv).float(), n, S, nh, dh)
    got = dict(o=heads(pick(fw["out"]).float(), n, S, nh, dh), lse=fw["lse"].view(B, nh, S)[sel], dq=dq, dk=dk, dv=dv)
    judge(got, ref, dh, f"many workgroups dh={dh} B={B}")


# ------------------------------------------------------------------------------------------------------------------ the CPU measurement
def measure():
    """worst floored row error of `restate` against `reference` over every host input of this module, per head width (run on the CPU; prints the
    figures the bounds above are three / four times of)"""
    worst = {dh: dict(fwd=(0.0, None), bwd=(0.0, None), lse=(0.0, None)) for dh in DHS}

    def note(dh, key, e, tag):
        if e > worst[dh][key][0]:
            worst[dh][key] = (e, tag)

    def one(dh, qkv, do, B, S, nh, fac, tag):
        ref, res = reference(qkv, do, B, S, nh, dh, fac), restate(qkv, do, B, S, nh, dh, fac)
        note(dh, "fwd", row_err(res["o"], ref["o"]), tag)
        note(dh, "lse", (res["lse"].double() - ref["lse"]).abs().max().item(), tag)
        for name in ("dq", "dk", "dv"):
            note(dh, "bwd", row_err(res[name], ref[name], ref["mag_" + name] if name != "dv" else None), tag + " " + name)

    for dh, S, kind, p, seed in host_cases():
        qkv, do, fac, _ = case_data(dh, S, kind, p, seed)
        one(dh, qkv, do, B0, S, NH0, fac, f"S={S} {kind} p={p}")
    for dh in DHS:                                                  # the many-workgroup shape, host-drawn
        g = torch.Generator().manual_seed(dh)
        qkv, do = torch.randn(3 * MANY_S, 6 * dh, generator=g).bfloat16(), torch.randn(3 * MANY_S, 2 * dh, generator=g).bfloat16()
        one(dh, qkv, do, 3, MANY_S, 2, drop_fac(P_DROP, 1234 + dh, range(3), 2, MANY_S, CPU), f"many S={MANY_S}")
    for dh, S in CASES_POS:
        qkv, _ = inputs(dh, B0, S, NH0, "half")
        fac = drop_fac(P_DROP, 0x9E3779B1, range(B0), NH0, S, CPU)
        for c in range((S + dh - 1) // dh):
            x, _w = one_hot_v(qkv, B0, S, NH0, dh, c)
            note(dh, "fwd", row_err(restate(x, None, B0, S, NH0, dh, fac, grad=False)["o"], reference(x, None, B0, S, NH0, dh, fac, grad=False)["o"]),
                 f"one-hot v S={S} block {c}")
    return worst


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))       # what tests/conftest.py does for a pytest run
    for dh, w in measure().items():
        for key, (e, tag) in w.items():
            print(f"head_dim {dh} {key}: {e:.3e}   at {tag}")
