"""Every attention kernel form against an fp64 statement of the operation (GPU).

Dispatch of clibd_attention_fwd / clibd_attention_bwd / clibd_attention_bwd_sp, read from the host code of csrc/attention.hip.
N = 2 * ceil(S / 32) key tiles of 16 (S 1..32 -> 2, 33..64 -> 4, ... 225..256 -> 16); MASK = key_mask given, DROP = drop_thr16 > 0; every row
exists for the four (MASK, DROP) pairs unless stated.  CUs = multi_processor_count of the device (read at run time, never assumed).

  row         condition (first match wins)                         instantiation                                         cases below
  F-persist   N >= 12 and B * nheads >= 2 * CUs, except MASK with   attention_fwd_persistent_kernel<N, MASK, DROP>        c (nq1-mask / nq17-mask at S = 197 are the excepted form: per-head), b at
              (N = 12 and DROP) or (N = 14 and no DROP)                                                                  S = 197 with 2 CUs + 5 heads
  F-3w        N == 10, 128 < S <= 144, nq > 128                    attention_fwd_kernel<10, false, MASK, DROP, 3, 144>   a at S = 129, 133, 144; b at 133; d at 129, 133; e at nq = 129
  F-per-head  every other forward launch                           attention_fwd_kernel<N, PAIR = N >= 10, MASK, DROP>   a (PAIR false N <= 8, true at S = 145 .. 256); e at S = 133 / 144 with
                                                                                                                         nq <= 128 (PAIR, N = 10); b, d, f, g; the chunked launches of c
  B-3w        N == 10, S <= 144, no mask, any nq                   attention_bwd_kernel<10, false, false, DROP, 3, 144>  a at S = 129, 133, 144 without mask; e at S = 133 / 144 without mask
  B           every other two-phase backward launch                attention_bwd_kernel<N, PAIR = N >= 12, MASK, DROP>   a (PAIR at S >= 161; the masked four-wave form at S = 129 .. 144;
                                                                                                                         9 / 11 / 13 / 15 key tiles at S = 133, 161, 197, 225); e, f, g
  SP          S <= 224, np = ceil(ceil(S / 16) / 2)                attention_bwd_sp_kernel<DROP, NPT>, NPT = 5 for S in  d: NPT 5 at S = 129, 133, 160; 7 at 193, 197, 224; 0 at 1, 16, 100,
                                                                   129 .. 160, 7 for 193 .. 224, 0 (run time) otherwise  128, 161, 192
The environment knobs CLIBD_ATTN_FWD_WAVES / CLIBD_ATTN_BWD_WAVES (four-wave forms at nine tiles) are read once per process and are out of
scope here, as are the compile-time A/B switches of the file.

Reference: softmax(q k^T / 8) in fp64 with masked keys at -inf, times the oracle's dropout factor for element ((b * nh + h) * S + q) << 8 | key
(oracle.clibd_oracle.drop_factor: an independent statement of the mask the three kernels index in three different ways), times v; gradients by
torch autograd in fp64.  B = 2, nh = 3 cases are evaluated on the host, the many-head cases on the device for a sample of sequences.

Judgement, per (sequence, head): the 2-norm of the error of every 64-element row of out / dq / dk / dv over max(|ref row|, 0.25 * mean row norm of that
(sequence, head)); the worst row must meet the bound.  (Without the floor a dQ row of a peaked softmax, a cancellation to nearly zero, shows
relative errors near 1 for a correct bf16 evaluation.)  A (sequence, head) whose reference dq / dk is entirely zero (a single live key: dS = P o (dP -
delta) cancels exactly) has no norm to divide by: its rows are divided by the magnitude of what cancels, sum_k P (|dP| + |delta|) |k_k| / 8 (|q_q| for
dk), so the kernels' rounding of delta against dP (fp32 in the two-phase form, the bf16 rounding of P o F inside the saved output in the single-pass
form) is held to the same bound.  Any other all-zero reference (dO = 0, dv of a masked key) must be met exactly.

Bounds: `restate` below is the operation in fp32 torch with the kernels' rounding points (un-normalised exp2(c2 s - c2 max) times the drop factor
rounded to bf16 before @ v, the fp32 row sum dividing the fp32 result, out to bf16; backward: normalised P in fp32, dP = (dO V^T) o F,
delta = sum(P o dP), dS to bf16 before both products, P o F to bf16 before dV, outputs to bf16).  `python tests/test_attention_forms_gpu.py`
runs it on the CPU over every host-made input of this module (and host-drawn operands of the many-head shapes, whose own operands are drawn on the
device from the same distribution) and prints the worst floored row errors:
    forward  4.955e-03  (the one-hot v of the dropout-position test, S = 133, keys 128 .. 132: rows of five non-zero elements; randn operands give 2.4e-3 .. 3.7e-3)
    backward 5.541e-03  (dq at B = 2, S = 209, nh = 3, randn, no mask, p = 0.1)
    lse      1.679e-05  (absolute, log2 domain: S = 197 with one query row 30 times larger, where |lse| is in the hundreds)
FWD_BOUND / BWD_BOUND are 3 x those (the kernels' v_exp / v_log / reciprocal, the MFMA accumulation order and the single-pass delta from o_hi + o_lo
live in the margin; one misplaced element in a row of 64 is an error near 0.18), LSE_BOUND 4 x, never above the project's 2e-3.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64, FP8, U8, I32 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn, torch.uint8, torch.int32
LOG2E = 1.4426950408889634
CPU = torch.device("cpu")
PAD = 3                       # sentinel rows (elements for lse) in front of and behind every output
P_DROP = 0.1
FP8_SCALE = 1500.0            # not a power of two; |o| > 448 / 1500 = 0.2987 saturates (a few percent of the outputs at S = 197: asserted)
FWD_WORST, BWD_WORST, LSE_WORST = 4.955e-3, 5.541e-3, 1.679e-5      # measured on the CPU: see the docstring
FWD_BOUND, BWD_BOUND, LSE_BOUND = 3 * FWD_WORST, 3 * BWD_WORST, min(4 * LSE_WORST, 2e-3)


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ------------------------------------------------------------------------------------------------------------------ operands
KINDS = ["randn", "half", "x4", "x0.05", "bigrow", "do0", "q0"]


@functools.lru_cache(maxsize=None)
def inputs(B, S, nh, kind="randn"):
    """(qkv [B*S, 3H], dO [B*S, H]) as bf16 on the host, made once per shape and never modified: q, k, v and dO all different randn draws"""
    g = torch.Generator().manual_seed(100000 * KINDS.index(kind) + 1000 * S + 10 * B + nh)
    H = 64 * nh
    qkv, do = torch.randn(B * S, 3 * H, generator=g), torch.randn(B * S, H, generator=g)
    if kind == "half":
        qkv *= 0.5
    elif kind == "x4":
        qkv *= 4.0
    elif kind == "x0.05":
        qkv *= 0.05
    elif kind == "bigrow":                      # one query row 30 times larger: sequence 0 in the middle, sequence 1 the last (the clamped) row
        x = qkv.view(B, S, 3 * H)
        x[0, S // 2, :H] *= 30.0
        x[1, S - 1, :H] *= 30.0
    elif kind == "do0":
        do.zero_()
    elif kind == "q0":
        qkv.view(B, S, 3, H)[:, :, 0] = 0.0
    return qkv.bfloat16(), do.bfloat16()


def make_mask(kind, B, S):
    """int32 [B, S], 1 = attend"""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(7 * S + B)
    m = torch.ones(B, S, dtype=I32)
    if kind == "prefix":
        for b in range(B):
            m[b, max(1, (2 * S) // 3 if b % 2 == 0 else S - 1):] = 0
    elif kind in ("holes", "dead"):
        m = (torch.rand(B, S, generator=g) < 0.5).to(I32)
        for b in range(B):
            m[b, (S // 2 + b) % S] = 1                                   # at least one live key per sequence
        if kind == "dead":
            m[1] = 0                                                     # one sequence with no live key at all
    elif kind == "head32":
        m[:, : min(32, S - 4)] = 0                                       # the first two key tiles entirely masked (S = 20: the first one)
    elif kind == "one":
        m.zero_()
        for b in range(B):
            m[b, S - 1 - (b * (S // 2)) % S] = 1                         # exactly one live key: the last one / one in the middle
    else:
        raise ValueError(kind)
    return m


def split(qkv, B, S, nh):
    """[B*S, 3H] -> q, k, v each [B, nh, S, 64]"""
    return qkv.view(B, S, 3, nh, 64).permute(2, 0, 3, 1, 4)


def heads(t, B, n, nh):
    """[B*n, H] -> [B, nh, n, 64]"""
    return t.view(B, n, nh, 64).permute(0, 2, 1, 3)


def drop_fac(p, seed, seqs, nh, S, nq, where):
    """the oracle's 0 or 1 / (1 - p) for element ((b * nh + h) * S + q) << 8 | key of the (global) sequences `seqs`: [len(seqs), nh, nq, S]"""
    from oracle.clibd_oracle import drop_factor

    b = torch.as_tensor(list(seqs), dtype=torch.int64, device=where).view(-1, 1, 1, 1)
    h = torch.arange(nh, dtype=torch.int64, device=where).view(1, nh, 1, 1)
    q = torch.arange(nq, dtype=torch.int64, device=where).view(1, 1, nq, 1)
    key = torch.arange(S, dtype=torch.int64, device=where).view(1, 1, 1, S)
    return drop_factor(seed, (((b * nh + h) * S + q) << 8) | key, p).to(where)


# ------------------------------------------------------------------------------------------------------------------ the two statements
def reference(qkv, do, B, S, nh, nq, mask, fac, grad=True):
    """fp64: out [B, nh, nq, 64], lse (log2 domain) [B, nh, nq], and dq, dk, dv [B, nh, S, 64] by autograd.  Plain: no rounding anywhere."""
    x = qkv.double().requires_grad_(grad)
    q, k, v = split(x, B, S, nh)
    s = (q[:, :, :nq] @ k.transpose(-1, -2)) * 0.125
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if fac is not None:
        p = p * fac.double()
    o = p @ v
    r = dict(o=o.detach(), lse=(torch.logsumexp(s, dim=-1) * LOG2E).detach())
    if grad:
        doh = heads(do.double(), B, nq, nh)
        (gx,) = torch.autograd.grad(o, x, doh)
        r["dq"], r["dk"], r["dv"] = split(gx, B, S, nh)
        with torch.no_grad():       # what cancels in dS = P o (dP - delta): the scale of dq / dk rows where the statement itself is exactly zero
            pd = torch.softmax(s, dim=-1)
            dp = doh @ v.transpose(-1, -2) * (1.0 if fac is None else fac.double())
            w = pd * (dp.abs() + (pd * dp).sum(-1, keepdim=True).abs())
            r["mag_dq"] = torch.zeros(B, nh, S, dtype=F64, device=qkv.device)
            r["mag_dq"][:, :, :nq] = 0.125 * (w @ k.norm(dim=-1, keepdim=True)).squeeze(-1)
            r["mag_dk"] = 0.125 * (w.transpose(-1, -2) @ q[:, :, :nq].norm(dim=-1, keepdim=True)).squeeze(-1)
    return r


def bfr(t):
    return t.bfloat16().float()


def restate(qkv, do, B, S, nh, nq, mask, fac, grad=True):
    """fp32 with the kernels' rounding points (see the docstring); same results layout as `reference`.  Only used to derive the bounds."""
    c2 = torch.tensor(0.125, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    q, k, v = split(qkv.float(), B, S, nh)
    q = q[:, :, :nq]
    s = q @ k.transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    mc = s.amax(-1, keepdim=True) * c2
    e = torch.exp2(s * c2 - mc)
    tot = e.sum(-1, keepdim=True)
    f = torch.ones((), dtype=F32) if fac is None else fac.float()
    r = dict(o=bfr((bfr(e * f) @ v) / tot), lse=(mc + torch.log2(tot)).squeeze(-1))
    if grad:
        doh = heads(do.float(), B, nq, nh)
        p = e / tot
        dp = (doh @ v.transpose(-1, -2)) * f
        ds = bfr(p * (dp - (p * dp).sum(-1, keepdim=True)))
        r["dq"] = torch.zeros(B, nh, S, 64)
        r["dq"][:, :, :nq] = bfr((ds @ k) * 0.125)
        r["dk"] = bfr((ds.transpose(-1, -2) @ q) * 0.125)
        r["dv"] = bfr(bfr(p * f).transpose(-1, -2) @ doh)
    return r


def row_err(got, ref, zero_floor=None):
    """worst 64-element row of |got - ref| / max(|ref row|, 0.25 * mean row norm of its (sequence, head)); inputs [..., rows, 64].
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
def nan_buf(dev, dtype, *shape):
    if dtype == FP8:
        return torch.full(shape, 0x7F, dtype=U8, device=dev).view(FP8)        # 0x7f: e4m3's NaN
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def is_nan(t):
    return (t.view(U8) & 0x7F) == 0x7F if t.dtype == FP8 else torch.isnan(t)


def guarded(dev, dtype, rows, *cols):
    """(buffer, view): `rows` NaN rows between PAD sentinel rows on either side"""
    buf = nan_buf(dev, dtype, rows + 2 * PAD, *cols)
    return buf, buf[PAD:PAD + rows]


def sentinels_intact(buf):
    return bool(is_nan(buf[:PAD]).all()) and bool(is_nan(buf[-PAD:]).all())


def run_fwd(ops, dev, qkv, B, S, nh, mask=None, nq=None, drop=None, fp8=0.0, save=False, out_seq=None):
    """one forward launch into NaN-filled, sentinel-guarded buffers; out_seq != nq goes through the C ABI directly (the wrapper passes nq, nq)"""
    H = 64 * nh
    nq = S if nq is None else nq
    out_seq = nq if out_seq is None else out_seq
    r, bufs = {}, []
    b, r["out"] = guarded(dev, FP8 if fp8 > 0 else BF16, B * out_seq, H)
    bufs.append(b)
    kw = {}
    if save:
        b, r["lse"] = guarded(dev, F32, B * nh * S)
        bufs.append(b)
        b, r["o_lo"] = guarded(dev, BF16, B * S, H)
        bufs.append(b)
        kw = dict(lse=r["lse"], o_lo=r["o_lo"])
    qkv, mask = qkv.to(dev), None if mask is None else mask.to(dev)
    if out_seq == nq:
        ops.attention_fwd(qkv, B, S, nh, mask, r["out"], nq=nq, drop=drop, out_fp8_scale=fp8, **kw)
    else:
        from clibd_amd import _lib

        _lib.check(_lib.load().clibd_attention_fwd(qkv.data_ptr(), B, S, nh, None if mask is None else mask.data_ptr(), r["out"].data_ptr(), nq, out_seq,
                                                   *ops._drop_args(drop), float(fp8), None, None, ops._stream()), "attention_fwd")
    torch.cuda.synchronize()
    assert all(sentinels_intact(b) for b in bufs), "forward wrote outside its buffers"
    live = r["out"].view(B, out_seq, H)
    assert not bool(is_nan(live[:, :nq]).any()), "forward left output rows unwritten (or NaN)"
    assert bool(is_nan(live[:, nq:]).all()), "forward wrote rows between nq and out_seq"
    if fp8 == 0:
        assert bool(torch.isfinite(live[:, :nq].float()).all())
        r["out"] = live[:, :nq].reshape(B * nq, H)
    else:
        r["out"] = live[:, :nq].reshape(B * nq, H).float() / fp8
    if save:
        assert bool(torch.isfinite(r["lse"]).all()) and bool(torch.isfinite(r["o_lo"].float()).all())
    return r


def run_bwd(ops, dev, qkv, do, B, S, nh, mask=None, nq=None, drop=None, dout_seq=None, sp=None):
    """one backward launch (two-phase; single-pass when `sp` holds the saving forward's outputs); dout_seq != nq through the C ABI with NaN rows
    between nq and dout_seq of every sequence's dO (they must never be read)"""
    H = 64 * nh
    nq = S if nq is None else nq
    dout_seq = nq if dout_seq is None else dout_seq
    buf, dqkv = guarded(dev, BF16, B * S, 3 * H)
    qkv, do, mask = qkv.to(dev), do.to(dev), None if mask is None else mask.to(dev)
    if sp is not None:
        ops.attention_bwd_sp(qkv, do, sp["out"], sp["o_lo"], sp["lse"], B, S, nh, dqkv, drop=drop)
    elif dout_seq == nq:
        ops.attention_bwd(qkv, do, B, S, nh, mask, dqkv, nq=nq, drop=drop)
    else:
        from clibd_amd import _lib

        wide = nan_buf(dev, BF16, B, dout_seq, H)
        wide[:, :nq] = do.view(B, nq, H)
        _lib.check(_lib.load().clibd_attention_bwd(qkv.data_ptr(), wide.data_ptr(), B, S, nh, None if mask is None else mask.data_ptr(), dqkv.data_ptr(),
                                                   nq, dout_seq, *ops._drop_args(drop), ops._stream()), "attention_bwd")
    torch.cuda.synchronize()
    assert sentinels_intact(buf), "backward wrote outside dqkv"
    assert bool(torch.isfinite(dqkv.float()).all()), "backward left rows unwritten (or not finite)"
    return dqkv


# ------------------------------------------------------------------------------------------------------------------ host-evaluated cases
def case_data(B, S, nh, kind, nq, mask_kind, p, seed):
    """operands, mask, drop factors and the fp64 reference of one host case (everything the CPU measurement needs as well)"""
    qkv, do_full = inputs(B, S, nh, kind)
    nq = S if nq is None else nq
    do = do_full.view(B, S, 64 * nh)[:, :nq].reshape(B * nq, 64 * nh).contiguous()
    mask = make_mask(mask_kind, B, S)
    thr = int(round(p * 65536.0))
    fac = drop_fac(p, seed & 0xFFFFFFFF, range(B), nh, S, nq, CPU) if thr > 0 else None
    live = [b for b in range(B) if mask is None or bool(mask[b].any())]
    return qkv, do, nq, mask, fac, live


def judge(got, ref, live, nq, tag):
    """forward / backward results (dicts of [B, nh, rows, 64]) against the reference on the sequences that have a live key"""
    if "o" in got:
        e = row_err(got["o"][live], ref["o"][live])
        assert e < FWD_BOUND, (tag, "out", e)
    if "dq" in got:
        assert bool((got["dq"][:, :, nq:] == 0).all()), (tag, "dq rows at and beyond nq must be exactly zero")
        for name in ("dq", "dk", "dv"):
            rows = slice(0, nq) if name == "dq" else slice(None)
            floor = ref["mag_" + name][live][:, :, rows] if name != "dv" else None
            e = row_err(got[name][live][:, :, rows], ref[name][live][:, :, rows], floor)
            assert e < BWD_BOUND, (tag, name, e)


def check(ops, dev, S, B=2, nh=3, kind="randn", nq=None, mask_kind=None, p=0.0, seed=None, out_seq_extra=0):
    """forward and two-phase backward of one host case against fp64, per row"""
    seed = 4242 + S if seed is None else seed
    qkv, do, nq, mask, fac, live = case_data(B, S, nh, kind, nq, mask_kind, p, seed)
    ref = reference(qkv, do, B, S, nh, nq, mask, fac)
    drop = ops.Drop(p, seed) if p > 0 else None
    tag = f"S={S} B={B} nh={nh} {kind} nq={nq} mask={mask_kind} p={p}"
    fw = run_fwd(ops, dev, qkv, B, S, nh, mask, nq, drop, out_seq=nq + out_seq_extra)
    dqkv = run_bwd(ops, dev, qkv, do, B, S, nh, mask, nq, drop, dout_seq=nq + out_seq_extra)
    dq, dk, dv = split(dqkv.cpu().float(), B, S, nh)
    got = dict(o=heads(fw["out"].cpu().float(), B, nq, nh), dq=dq, dk=dk, dv=dv)
    judge(got, ref, live, nq, tag)
    return got, ref, (qkv, do, mask)


def tiles_edges(N):
    return [16 * (N - 2) + 1, 16 * (N - 1), 16 * (N - 1) + 1, 16 * N]


S_A = sorted({s for N in range(2, 17, 2) for s in tiles_edges(N)} | {133, 197})
CASES_A = [(S, mk, p) for S in S_A for mk in (None, "prefix") for p in (0.0, P_DROP)]
S_D = [1, 16, 100, 128, 129, 133, 160, 161, 192, 193, 197, 224]
CASES_D = [(S, p) for S in S_D for p in (0.0, P_DROP)]
CASES_E = [(S, nq, mk) for S in (64, 133, 144, 197) for nq in (1, 16, 17, 33, 129) if nq <= S for mk in (None, "prefix")]
CASES_E_ABI = [(133, 129, None), (197, 17, "prefix")]          # (S, nq, mask) with out_seq = dout_seq = nq + 3
CASES_F = [(mk, S) for mk in ("holes", "head32", "one", "dead") for S in (20, 133, 197)]
CASES_G = [(kind, S) for kind in ("x4", "x0.05", "bigrow", "do0", "q0") for S in (64, 133, 197)]
CASES_B = [(20, None, 20), (80, None, 80), (133, None, 133), (197, None, 197), (256, None, 256), (133, "prefix", 99), (80, None, 0x9E3779B1)]   # (S, mask, seed)
S_C7 = [161, 197, 256]                                           # 7 CUs + 5 heads
MANY = {                                                         # 2 CUs + 5 heads: name -> (S, mask, p, nq, fp8, save)
    "S176-mask": (176, "prefix", 0.0, None, False, False), "S192-mask": (192, "prefix", 0.0, None, False, False),
    "S193-drop": (193, None, P_DROP, None, False, False), "S224-mask-drop": (224, "prefix", P_DROP, None, False, False),
    "nq1": (197, None, 0.0, 1, False, False), "nq1-mask": (197, "prefix", 0.0, 1, False, False),
    "nq17": (197, None, 0.0, 17, False, False), "nq17-mask": (197, "prefix", 0.0, 17, False, False),
    "nq1-mask-S176": (176, "prefix", 0.0, 1, False, False),          # (masked twelve-tile form: persistent, where S = 197 masked without dropout is not)
    "fp8": (197, None, 0.0, None, True, False), "save-drop": (197, None, P_DROP, None, False, True),
}


def host_cases():
    """every (B, S, nh, kind, nq, mask, p, seed) the host-evaluated tests use: the inputs the bounds are measured on"""
    for S, mk, p in CASES_A:
        yield 2, S, 3, "randn", None, mk, p, 4242 + S
    for S, p in CASES_D:
        yield 2, S, 3, "randn", None, None, p, 777 + S
    for S, nq, mk in CASES_E + CASES_E_ABI:
        yield 2, S, 3, "randn", nq, mk, 0.0, 0
    for mk, S in CASES_F:
        yield (3 if mk == "dead" else 2), S, 3, "randn", None, mk, 0.0, 0
    for kind, S in CASES_G:
        yield 2, S, 3, kind, None, None, 0.0, 0
    for S in sorted(set(S_C7) | {v[0] for v in MANY.values()}):           # the many-head shapes, host-drawn
        for mk in (None, "prefix"):
            for p in (0.0, P_DROP):
                yield 2, S, 12, "randn", None, mk, p, 4242 + S


# ---- a. per-head forward and two-phase backward: all eight tile counts
@pytest.mark.parametrize("S,mask_kind,p", CASES_A, ids=[f"S{S}-{mk or 'nomask'}-p{p}" for S, mk, p in CASES_A])
def test_every_tile_count(ops, dev, S, mask_kind, p):
    """N = 2 .. 16 at the lower edge of the tile count, on both sides of the `last_live` boundary and at the full image, {mask} x {dropout};
    S = 1 is a single key (dS, and with it the statement's dq and dk, exactly zero: judged against the magnitude of what cancels)."""
    got, ref, _ = check(ops, dev, S, mask_kind=mask_kind, p=p)
    if S == 1:
        assert float(ref["dq"].abs().max()) == 0.0 and float(ref["dk"].abs().max()) == 0.0


# ---- b. dropout positions, exactly
def one_hot_v(qkv, B, S, nh, c):
    """v of key 64 c + d is the unit vector e_d (every other key's v is zero): out[q, d] reads P[q, 64 c + d] * F[q, 64 c + d] back"""
    x = qkv.clone().view(B, S, 3, nh, 64)
    x[:, :, 2] = 0
    w = min(64, S - 64 * c)
    d = torch.arange(w, device=qkv.device)
    x[:, 64 * c + d, 2, :, d] = 1.0
    return x.view(B * S, 3 * 64 * nh), w


def check_positions(out, fac, ref, mask, c, w, tag):
    """out [B, nh, S, 64] (fp32), fac [B, nh, S, S]: the zero set of columns 0 .. w-1 is exactly the oracle's dropped (or masked) set of keys
    64 c .. 64 c + w - 1, the columns without a key are zero, and the values meet the forward bound"""
    gone = fac[..., 64 * c:64 * c + w] == 0
    if mask is not None:
        gone = gone | (mask[:, None, None, 64 * c:64 * c + w] == 0)
    assert torch.equal(out[..., :w] == 0, gone), (tag, c, int(((out[..., :w] == 0) != gone).sum()))
    assert bool((out[..., w:] == 0).all()), (tag, c)
    assert 0.03 < float(fac[..., 64 * c:64 * c + w].eq(0).double().mean()) < 0.2, tag              # the mask is a mask of p = 0.1
    e = row_err(out, ref["o"])
    assert e < FWD_BOUND, (tag, c, e)


@pytest.mark.parametrize("S,mask_kind,seed", CASES_B, ids=[f"S{S}-{mk or 'nomask'}-seed{seed:x}" for S, mk, seed in CASES_B])
def test_dropout_positions_forward(ops, dev, S, mask_kind, seed):
    """Per-head (S = 20, 80, 197, 256) and three-wave (133) forward: which probabilities are dropped, element by element, against the oracle's hash
    of ((head * S + q) << 8) | key; once with a key mask, once with a seed whose high bit is set."""
    B, nh = 2, 3
    qkv, _ = inputs(B, S, nh, "half")
    mask = make_mask(mask_kind, B, S)
    drop = ops.Drop(P_DROP, seed)
    fac = drop_fac(P_DROP, drop.seed, range(B), nh, S, S, CPU)
    for c in range((S + 63) // 64):
        x, w = one_hot_v(qkv, B, S, nh, c)
        ref = reference(x, None, B, S, nh, S, mask, fac, grad=False)
        out = heads(run_fwd(ops, dev, x, B, S, nh, mask, drop=drop)["out"].cpu().float(), B, S, nh)
        check_positions(out, fac, ref, mask, c, w, f"S={S} mask={mask_kind} seed={seed:#x}")


# ---- c. persistent forward
def sample_sequences(B, nh, cus):
    """the first and the last sequence and those holding heads k * CUs - 1 and k * CUs of every round k of the persistent walk"""
    total = B * nh
    seqs = {0, B - 1}
    for k in range(1, (total - 1) // cus + 1):
        seqs |= {(k * cus - 1) // nh, (k * cus) // nh}
    return sorted(seqs)


def device_operands(dev, B, S, nh, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(B * S, 3 * 64 * nh, generator=g, device=dev).bfloat16()


def chunked_per_head(ops, dev, cus, qkv, B, S, nh, mask, nq, fp8):
    """the same forward through the per-head kernel: consecutive batch chunks of fewer than 2 CUs heads"""
    chunk = (2 * cus - 1) // nh
    assert chunk >= 1 and chunk * nh < 2 * cus
    outs = []
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        m = None if mask is None else mask[b0:b1].contiguous()
        outs.append(run_fwd(ops, dev, qkv[b0 * S:b1 * S], b1 - b0, S, nh, m, nq, None, fp8)["out"])
    return torch.cat(outs)


def check_many_heads(ops, dev, cus, rounds, S, mask_kind=None, p=0.0, nq=None, fp8=False, save=False):
    nh = 12
    B = -(-(rounds * cus + 5) // nh)
    if (B * nh) % cus == 0:
        B += 1                                                     # the last round must be ragged
    assert B * nh >= rounds * cus + 5 and B * nh >= 2 * cus and S > 160        # the persistent kernel's condition
    nq_ = S if nq is None else nq
    tag = f"persistent S={S} B={B} mask={mask_kind} p={p} nq={nq} fp8={fp8} save={save}"
    qkv = device_operands(dev, B, S, nh, S + rounds)
    mask = None
    if mask_kind is not None:
        lens = torch.randint(max(1, S // 3), S + 1, (B,), generator=torch.Generator().manual_seed(S))
        mask = (torch.arange(S)[None, :] < lens[:, None]).to(I32).to(dev)
    drop = ops.Drop(p, 1234 + S) if p > 0 else None
    scale = FP8_SCALE if fp8 else 0.0
    fw = run_fwd(ops, dev, qkv, B, S, nh, mask, nq, drop, scale, save)
    if p == 0:                                                     # dropout indices follow the global head: chunks would shift them
        same = chunked_per_head(ops, dev, cus, qkv, B, S, nh, mask, nq, scale)
        assert torch.equal(fw["out"], same), (tag, "persistent and per-head kernels differ", int((fw["out"] != same).any(dim=1).sum()))
    seqs = sample_sequences(B, nh, cus)
    n = len(seqs)
    sel = torch.as_tensor(seqs, device=dev)
    qs = qkv.view(B, S, -1)[sel].reshape(n * S, -1)
    ms = None if mask is None else mask[sel]
    fac = drop_fac(p, drop.seed, seqs, nh, S, nq_, dev) if p > 0 else None
    ref = reference(qs, None, n, S, nh, nq_, ms, fac, grad=False)
    out = heads(fw["out"].view(B, nq_, -1)[sel].reshape(n * nq_, -1).float(), n, nq_, nh)
    if fp8:
        check_fp8(out, ref["o"], tag)
    else:
        e = row_err(out, ref["o"])
        assert e < FWD_BOUND, (tag, e)
    if save:
        check_saved(fw["lse"].view(B, nh, S)[sel], heads(fw["o_lo"].view(B, S, -1)[sel].reshape(n * S, -1).float(), n, S, nh), out, ref, tag)


def check_fp8(dec, ref, tag):
    """e4m3(o * scale) / scale against fp64: half an e4m3 step of the (clamped) reference, half a subnormal step, and the forward bound on the row"""
    lim = 448.0 / FP8_SCALE
    frac = float((ref.abs() > lim).double().mean())
    assert 0.005 < frac < 0.2, (tag, "the scale should saturate a few percent of the outputs", frac)
    rc = ref.clamp(-lim, lim)
    n = ref.norm(dim=-1, keepdim=True)
    tol = rc.abs() * 2.0 ** -4 + 2.0 ** -10 / FP8_SCALE + FWD_BOUND * torch.maximum(n, 0.25 * n.mean(dim=-2, keepdim=True))
    over = ((dec.double() - rc).abs() / tol).max().item()
    assert over <= 1.0, (tag, over)


def check_saved(lse, o_lo, out, ref, tag):
    """the saving forward: lse (log2 domain) and the two invariants of the rounding residual"""
    e = (lse.double() - ref["lse"]).abs().max().item()
    assert e < LSE_BOUND, (tag, "lse", e)
    assert bool((o_lo.abs() <= out.abs() * 2.0 ** -8).all()), (tag, "o_lo is at most half an ulp of out")
    e_hi, e_sum = row_err(out, ref["o"]), row_err(out.double() + o_lo.double(), ref["o"])
    assert e_sum <= 1.05 * e_hi + 1e-5, (tag, e_hi, e_sum)


@pytest.mark.parametrize("S", S_C7)
def test_persistent_forward_seven_rounds(ops, dev, cus, S):
    """>= 7 CUs + 5 heads: every workgroup walks it = 0 .. 6 (the tile rotation (wave + 3 it) & 15 wraps at it = 6, both K / V buffers are handed over
    three times, queries are prefetched a head ahead, the partial vmcnt wait follows a head that stored) and the last round is ragged.  fp64 on the
    sequences around every round boundary, and every output bit against the per-head kernel."""
    check_many_heads(ops, dev, cus, 7, S)


@pytest.mark.parametrize("name", list(MANY))
def test_persistent_forward_forms(ops, dev, cus, name):
    """2 CUs + 5 heads through the other instantiations and stores of the persistent kernel: mask, dropout, both, nq = 1 / 17 (with mask: the
    [CLS]-only last text block), e4m3 output, lse / o_lo under dropout."""
    S, mask_kind, p, nq, fp8, save = MANY[name]
    check_many_heads(ops, dev, cus, 2, S, mask_kind, p, nq, fp8, save)


def test_dropout_positions_persistent(ops, dev, cus):
    """S = 197 on the persistent kernel (index from the walked head, not blockIdx): the dropped set of the sampled sequences, exactly."""
    S, nh = 197, 12
    B = -(-(2 * cus + 5) // nh)
    qkv = device_operands(dev, B, S, nh, 5) * 0.5
    drop = ops.Drop(P_DROP, 31337)
    seqs = sample_sequences(B, nh, cus)
    n, sel = len(seqs), torch.as_tensor(seqs, device=dev)
    fac = drop_fac(P_DROP, drop.seed, seqs, nh, S, S, dev)
    for c in range((S + 63) // 64):
        x, w = one_hot_v(qkv, B, S, nh, c)
        out = run_fwd(ops, dev, x, B, S, nh, drop=drop)["out"]
        xs = x.view(B, S, -1)[sel].reshape(n * S, -1)
        ref = reference(xs, None, n, S, nh, S, None, fac, grad=False)
        check_positions(heads(out.view(B, S, -1)[sel].reshape(n * S, -1).float(), n, S, nh), fac, ref, None, c, w, f"persistent positions S={S}")


def test_fp8_output_per_head_pair_sweep(ops, dev):
    """e4m3 output of the per-head kernel's two stores (one-tile sweep at S = 100, PAIR sweep at S = 197, three-wave at 133), clamp included"""
    for S in (100, 133, 197):
        qkv, do, nq, mask, fac, live = case_data(2, S, 3, "randn", None, None, 0.0, 0)
        ref = reference(qkv, None, 2, S, 3, S, None, None, grad=False)
        out = heads(run_fwd(ops, dev, qkv, 2, S, 3, fp8=FP8_SCALE)["out"].cpu(), 2, S, 3)
        check_fp8(out, ref["o"], f"fp8 S={S}")


# ---- d. single-pass backward
@pytest.mark.parametrize("S,p", CASES_D, ids=[f"S{S}-p{p}" for S, p in CASES_D])
def test_single_pass_backward(ops, dev, S, p):
    """The saving forward (lse, o_lo) and attention_bwd_sp built on it, against fp64 per row; NPT = 5, 7 and the run-time form on both sides of
    their edges; a second call gives the same bits."""
    B, nh, seed = 2, 3, 777 + S
    qkv, do, nq, mask, fac, live = case_data(B, S, nh, "randn", None, None, p, seed)
    ref = reference(qkv, do, B, S, nh, S, None, fac)
    drop = ops.Drop(p, seed) if p > 0 else None
    tag = f"single pass S={S} p={p}"
    fw = run_fwd(ops, dev, qkv, B, S, nh, drop=drop, save=True)
    plain = run_fwd(ops, dev, qkv, B, S, nh, drop=drop)
    assert torch.equal(plain["out"], fw["out"]), (tag, "the saving forward changes out")
    out = heads(fw["out"].cpu().float(), B, S, nh)
    check_saved(fw["lse"].cpu().view(B, nh, S), heads(fw["o_lo"].cpu().float(), B, S, nh), out, ref, tag)
    dqkv = run_bwd(ops, dev, qkv, do, B, S, nh, drop=drop, sp=fw)
    dq, dk, dv = split(dqkv.cpu().float(), B, S, nh)
    judge(dict(o=out, dq=dq, dk=dk, dv=dv), ref, live, S, tag)
    again = run_bwd(ops, dev, qkv, do, B, S, nh, drop=drop, sp=fw)
    assert torch.equal(again, dqkv), (tag, "not reproducible")


def test_single_pass_backward_rejects_225(ops, dev):
    S = 225
    z = torch.zeros((S, 3 * 64), dtype=BF16, device=dev)
    o = torch.zeros((S, 64), dtype=BF16, device=dev)
    with pytest.raises(RuntimeError, match="224"):
        ops.attention_bwd_sp(z, o, o, o, torch.zeros(S, device=dev), 1, S, 1, torch.empty_like(z))


# ---- e. query prefix
@pytest.mark.parametrize("S,nq,mask_kind", CASES_E, ids=[f"S{S}-nq{nq}-{mk or 'nomask'}" for S, nq, mk in CASES_E])
def test_query_prefix(ops, dev, S, nq, mask_kind):
    """Only the first nq queries: out is [B * nq, H], dq rows at and beyond nq are exactly zero (asserted in `judge`), dk / dv are those of the first nq
    queries; with a mask (the [CLS]-only last text block at nq = 1) and without."""
    check(ops, dev, S, nq=nq, mask_kind=mask_kind)


@pytest.mark.parametrize("S,nq,mask_kind", CASES_E_ABI, ids=[f"S{S}-nq{nq}-{mk or 'nomask'}" for S, nq, mk in CASES_E_ABI])
def test_query_prefix_wider_row_stride(ops, dev, S, nq, mask_kind):
    """out_seq = dout_seq = nq + 3 through the C ABI (the wrapper always passes nq): rows nq .. out_seq - 1 of every sequence stay NaN (asserted in
    `run_fwd`), and the NaN rows of dO in the same places are never read."""
    check(ops, dev, S, nq=nq, mask_kind=mask_kind, out_seq_extra=3)


# ---- f. masks
@pytest.mark.parametrize("mask_kind,S", CASES_F, ids=[f"{mk}-S{S}" for mk, S in CASES_F])
def test_mask_shapes(ops, dev, mask_kind, S):
    """Masks that are not prefixes: random holes, the first key tiles entirely masked, a single live key (dS exactly zero in the statement), and a batch with one
    entirely masked sequence — that sequence is only required to come back finite (include/clibd_hip.h), its neighbours meet the bounds.
    (Found at S = 133 and 197: keys 0, 4, 8 and 12 were never masked in the forms of ten and more key tiles, and the dead sequence came back NaN.)"""
    got, ref, _ = check(ops, dev, S, B=3 if mask_kind == "dead" else 2, mask_kind=mask_kind)
    if mask_kind == "one":
        assert float(ref["dq"].abs().max()) == 0.0 and float(ref["dk"].abs().max()) == 0.0


# ---- g. value edges
@pytest.mark.parametrize("kind,S", CASES_G, ids=[f"{k}-S{S}" for k, S in CASES_G])
def test_value_edges(ops, dev, kind, S):
    """Peaked (x 4) and flat (x 0.05) softmax, one query row 30 times larger than the rest, dO = 0 (dqkv exactly zero), q = 0 (out = mean of v)."""
    got, ref, (qkv, do, mask) = check(ops, dev, S, kind=kind)
    if kind == "do0":
        assert all(float(got[n].abs().max()) == 0.0 for n in ("dq", "dk", "dv"))
    if kind == "q0":
        v = split(qkv.double(), 2, S, 3)[2]
        e = row_err(got["o"], v.mean(dim=2, keepdim=True).expand_as(v))
        assert e < FWD_BOUND, e


# ------------------------------------------------------------------------------------------------------------------ the CPU measurement
def measure():
    """worst floored row error of `restate` against `reference` over every host input of this module (run on the CPU; prints the figures the
    bounds above are three / four times of)"""
    worst = dict(fwd=(0.0, None), bwd=(0.0, None), lse=(0.0, None))

    def note(key, e, tag):
        if e > worst[key][0]:
            worst[key] = (e, tag)

    for B, S, nh, kind, nq, mk, p, seed in host_cases():
        qkv, do, nq, mask, fac, live = case_data(B, S, nh, kind, nq, mk, p, seed)
        ref, res = reference(qkv, do, B, S, nh, nq, mask, fac), restate(qkv, do, B, S, nh, nq, mask, fac)
        tag = f"B={B} S={S} nh={nh} {kind} nq={nq} mask={mk} p={p}"
        note("fwd", row_err(res["o"][live], ref["o"][live]), tag)
        note("lse", (res["lse"][live].double() - ref["lse"][live]).abs().max().item(), tag)
        for name in ("dq", "dk", "dv"):
            rows = slice(0, nq) if name == "dq" else slice(None)
            note("bwd", row_err(res[name][live][:, :, rows], ref[name][live][:, :, rows]), tag + " " + name)
    for S, mk, seed in CASES_B:
        qkv, _ = inputs(2, S, 3, "half")
        mask = make_mask(mk, 2, S)
        fac = drop_fac(P_DROP, seed & 0xFFFFFFFF, range(2), 3, S, S, CPU)
        for c in range((S + 63) // 64):
            x, _w = one_hot_v(qkv, 2, S, 3, c)
            note("fwd", row_err(restate(x, None, 2, S, 3, S, mask, fac, grad=False)["o"], reference(x, None, 2, S, 3, S, mask, fac, grad=False)["o"]),
                 f"one-hot v S={S} mask={mk} block {c}")
    return worst


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))       # what tests/conftest.py does for a pytest run
    for key, (e, tag) in measure().items():
        print(f"{key}: {e:.3e}   at {tag}")
