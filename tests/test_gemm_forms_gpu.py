"""Every bf16 GEMM kernel form, per element, against an fp64 statement of the operation from the same bf16 operands.

The operation, the restatement with the kernels' rounding points, the judgement and the case lists live in tests/gemm_reference.py
(CPU-importable; its docstring states the rounding points and how the magnitude sum `s` is carried).  This module launches every case
through clibd_amd.ops, with sentinels around every output and poison in every operand's padding.

DISPATCH TABLE (read from gemm.hip gemm_impl, gemm256.hip gemm256_try_launch / kernel_ptr / gemm256_splitk_launch, gemm_common.h
epilogue_kind, gemm256_tn.hip gemm256_tn_splitk_launch, gemm.hip tn_splitk_impl / transpose_impl / cast entries).  T = test below.

gemm_impl (clibd_gemm_bf16_nt, clibd_gemm_bf16_nt_khole)
  rejects (nothing launched)                                  null A/W/ep; bad hole; M,N,K <= 0; K % 64; N % 16; lda/ldw % 8 or < K; misaligned
                                                              operand / epilogue pointer; no output; rank_u xor rank_v; ld_rank_u; aux missing or
                                                              ld_aux (% 8, % 16 byte codes, % 4 e4m7); e4m7 with N % 8; SAVE_GRAD without out_pre;
                                                              act out of range; ld_res % 4; ld_pre; ld_out_bf16 % 8; ld_out_f32 % 4; dropout with
                                                              split_k > 1 / odd drop_ld; split_k > 1 with anything but a plain fp32 output;
                                                              a fold epilogue that gemm256 declines                         T rejections
                                                              (null pointers, rank_u xor rank_v, an odd drop_ld and e4m7 with N % 8 but N % 16 == 0
                                                              cannot be expressed through clibd_amd.ops, which raises before the call)
  row_sums / row_stats (fold)  -> gemm256_try_launch or error                                                              T 256_fold, rejections
  hole_len == 0 and gemm256_try_launch takes it -> 256x256 kernel                                                          T 256_*
  everything else -> gemm_bf16_nt_kernel (128x128), grid tiles_m x tiles_n x split                                         T 128_*
      store_row16: split_k > 1 (atomics) | dropout | SAVE_GRAD_E12 | SAVE_GRAD_U8 | SAVE_GRAD | out_pre | GELU | GELU_GRAD | MUL_AUX_E12 |
      MUL_AUX_U8 | MUL_AUX | ADD_AUX | residual | out_f32 | out_bf16; rank-8 k-step and bias on split 0 only; K hole in stage()
                                                                                                          T 128_epilogue, 128_split_k, 128_k_hole
gemm256_try_launch: K % 64 == 0, nk = K/64 >= 4 and even (K % 128 == 0, K >= 256); N % 256 == 0; split_k <= 1; M >= 1024; tiles >= 128;
  operands < 2^32 bytes; kind >= 0; kernel_ptr != null.  band = -CLIBD_WS_GROUP (W-stationary groups of 6 column tiles); grid = min(tiles, CUs);
  persistent loop over tile ids.                                       T 256_kinds (128 tiles, nk 4 and 6), 256_tile_order (tiles_n 3 < 6, 16 = 6+6+4,
                                                                         tiles > CUs, M = 1024), threshold_pairs (M 1023|1024, tiles 127|128)
  stream-K tail (workspace from the caller)                            out of scope: off unless CLIBD_GEMM_STREAMK=1 at import; own exactness test
epilogue_kind -> kernel_ptr(kind, lora, bias, diag=false): gemm256_bf16_nt_kernel<KIND, LORA, BIAS, false, false>
  BF16, F32, GELU, GELU_SAVE, GELU_SAVE_U8, GELU_SAVE_12, MUL_AUX, MUL_AUX_U8, MUL_AUX_12, ADD_AUX, RES_F32, RES_F32_DROP, GENERIC:
      x LORA {0,1} x BIAS {0,1}                                        T 256_kinds (all 13 x 4, K = 256 and 384), 256_strided, 256_scaled
      GENERIC's store_row8 branches: GELU_GRAD + residual + two outputs (256_kinds); out_pre + GELU + two outputs (256_strided)
  RES_F32_COPY <false, true> (row_sums), ROWNORM_GELU <false, true> (row_stats + col_sum_w): bias-only                     T 256_fold
  SPLITK_F32 <false, false>: gemm256_splitk_launch only                                                                    T nt_splitk
  kind -1 (an e4m7 act outside its two kinds; an inconsistent fold) -> declined: 128x128 kernel, or the fold's error      T 128_epilogue, rejections
  DIAG instantiations: diagnostic build only; CLIBD_GEMM_KERNEL=1: process-wide override                                  out of scope
gemm256_splitk_launch (clibd_gemm_bf16_nt_splitk): nk >= 8 and even, N % 256 == 0, M >= 1, workspace large enough; splits from plan_k_slices
  (CU count); partials -> reduce_splits_kernel (accumulate 0 | 1); returns 0 -> "shape not supported" -> False            T nt_splitk
tn_splitk_impl / gemm256_tn_splitk_launch (clibd_gemm_bf16_tn_splitk): M % 128 == 0, M >= 256, Na % 256 == 0, Nb % 256 == 0;
  gemm256_tn_kernel<COLSUM, false>; colsum by atomics | colsum workspace + ordered_colsum_kernel; reduce_splits_kernel    T tn_splitk
  b_scale > 0 (fp8 B), clibd_gemm_fp8_nt, clibd_gemm_fp8_dgrad_nt                                                         out of scope (test_fp8_gpu.py, test_dgrad8_gpu.py,
                                                                                                                           test_fp8_full_finetune_gpu.py)
transpose_impl: fast (C % 8 == 0, ld_in % 8 == 0, ld_out % 8 == 0, aligned): transpose_colsum_bf16_kernel<4> (ld_out >= 1024) | <1>;
  colsum: none | atomics | partials + colsum_partials_kernel; otherwise transpose_bf16_kernel (no colsum)                 T transpose_*
clibd_transpose_fp8_bf16, clibd_cast_f32_to_bf16 (vector body + n % 4 tail by one thread), clibd_cast_transpose_f32_to_bf16   T transpose_fp8, casts
The 2^32-byte operand fallback needs a 4 GB operand; the LoRA kernels are not GEMM forms: out of scope.

JUDGEMENT.  e = |got - ref| / max(|ref|, 2^-10 s) for every element of every output; the worst element must meet the bound of its class,
3 x the worst e of the CPU restatement over every input of this module (`python tests/test_gemm_forms_gpu.py`, saved as
profiles/gemm_forms_cpu_restatement.log; the margin is for the MFMA accumulation order, v_exp / v_rcp, and the order of atomics).  Classes:
bf16 and fp32 value outputs, fp32 accumulate outputs (split-K paths, column sums), gelu' as bf16 / decoded from the one-byte code / from e4m7,
row_sums — and, kept apart so that they do not set those bounds: outputs behind an intermediate bf16 rounding ("_mid": 2^-9 |x| is above the
floor), outputs behind ACT_GELU_GRAD ("_gg": the erf approximation's absolute error times the accumulator), and the fold consumer against the
UN-folded LayerNorm -> Linear -> GELU ("_fold": the fold rounds w gamma to bf16, the un-folded statement does not; the same launch is also
judged against the folded formula in fp64, in the ordinary classes).  The one-byte code also meets the derived bound of
test_gemm256_epilogue_kinds per element (gemm_reference.u8_derived_bound).  An all-zero reference (a dropped element without residual) is met exactly.

Measured on an MI355X (worst e over the module per class, against the bounds): see profiles/gemm_forms_mi355x.log."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import gemm_reference as G  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8

# worst e of the CPU restatement against fp64 per class (python tests/test_gemm_forms_gpu.py; profiles/gemm_forms_cpu_restatement.log)
WORST = {"bf16": 3.8955e-3, "f32": 9.8436e-5, "f32_acc": 5.5254e-5, "dg_bf16": 1.5536e-1, "dg_u8": 2.8187e-1, "dg_e12": 1.3458e-1,
         "row_sums": 4.0941e-6, "bf16_mid": 2.2386e-2, "f32_mid": 1.9808e-2, "bf16_gg": 1.9924e-2, "f32_gg": 2.0087e-2,
         "bf16_fold": 3.6889e-1, "dg_bf16_fold": 3.7819e-1}
BOUND = {k: 3.0 * v for k, v in WORST.items()}
U8_FILL = 0xA5


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.fixture(scope="module")
def seen():
    """worst e per class over the module, printed at the end (-s shows it)"""
    w = {}
    yield w
    print("\n[gemm forms] worst e per class on this device: " + ", ".join(f"{k} {v:.3e} (bound {BOUND[k]:.3e})" for k, v in sorted(w.items())))


# ------------------------------------------------------------------------------------------------ buffers
def _fill(dtype):
    return U8_FILL if dtype == U8 else float("nan")


def _bits(t):
    return t.view({BF16: torch.int16, F32: torch.int32, U8: torch.uint8}[t.dtype])


def guarded(dev, rows, width, ld, dtype):
    """an output of `rows` x `width` inside a sentinel-filled buffer: 3 rows before and after, columns up to the row stride `ld`"""
    big = torch.full((rows + 6, ld), _fill(dtype), dtype=dtype, device=dev)
    return big, big[3:3 + rows, :width]


def assert_guard_untouched(big, rows, width, what):
    b = _bits(big)
    pat = _bits(torch.full((1,), _fill(big.dtype), dtype=big.dtype, device=big.device))[0]
    ok = (b[:3] == pat).all() & (b[3 + rows:] == pat).all() & (b[3:3 + rows, width:] == pat).all()
    assert bool(ok), f"{what}: a sentinel outside [0, M) x [0, N) was overwritten"


def poisoned(t, ld):
    """operand `t` in a buffer of row stride `ld` whose padding columns are NaN (0xA5 for bytes)"""
    if ld == t.shape[1]:
        return t
    big = torch.full((t.shape[0], ld), _fill(t.dtype), dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def up16(n):
    return (n + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ one case
_ref_cache = {}


def launch(ops, dev, c, given=None, operands=None):
    """launch case `c`; returns {output name: (guard buffer, view, rows, width)} after checking nothing; operands absent from the case are null"""
    d = G.draws_for(c)
    M, N, K, sx = c.M, c.N, c.K, c.strided
    pad = lambda n, extra: n + (extra if sx else 0)
    if c.fold == "consumer":
        a, w = d.get("x1", dev).to(BF16), given["wg"]
    else:
        a, w = d.get("A", dev), d.get("W", dev)
        if c.hole and c.hole[1] > 0:     # NaN in both operands inside the hole: a hole that is read gives NaN
            k0, ln = c.hole
            a, w = a.clone(), w.clone()
            a[:, k0:k0 + ln] = float("nan")
            w[:, k0:k0 + ln] = float("nan")
        a, w = poisoned(a, pad(K, 8)), poisoned(w, pad(K, 8))
    kw = dict(act=c.act, split_k=c.split_k)
    if c.fold == "consumer":
        kw.update(bias=given["bp"], row_stats=given["stats"], col_sum_w=given["s_n"])
    elif c.bias:
        kw["bias"] = d.get("bias", dev)
    if c.rank:
        kw["rank_u"], kw["rank_v"] = poisoned(d.get("u", dev), 16), d.get("v", dev)      # ld_rank_u = 16 everywhere: NaN in columns 8 and up
    if c.aux == "bf16":
        kw["aux"] = poisoned(d.get("aux", dev), pad(N, 8))
    elif c.aux == "u8":
        kw["aux"] = poisoned(d.get("codes", dev), pad(N, 16))
    elif c.aux == "e12":
        kw["aux"] = poisoned(G.e12_pack(d.get("g12", dev)), pad(3 * N // 2, 16))
    if c.residual:
        kw["residual"] = poisoned(d.get("res", dev), pad(N, 4))
    if c.drop > 0:
        kw["drop"] = ops.Drop(*G.drop_site(c))
    if c.hole:
        kw["k_hole"] = c.hole
    outs = {}
    if c.has_pre:
        if c.act == G.ACT_GELU_SAVE_GRAD_U8:
            outs["out_pre"] = guarded(dev, M, N, pad(N, 16), U8) + (M, N)
        elif c.act == G.ACT_GELU_SAVE_GRAD_E12:
            outs["out_pre"] = guarded(dev, M, 3 * N // 2, up16(3 * N // 2) + (16 if sx else 0), U8) + (M, 3 * N // 2)
        else:
            outs["out_pre"] = guarded(dev, M, N, pad(N, 8), BF16) + (M, N)
    if c.out_bf16:
        outs["out_bf16"] = guarded(dev, M, N, pad(N, 8), BF16) + (M, N)
    if c.out_f32:
        outs["out_f32"] = guarded(dev, M, N, pad(N, 4), F32) + (M, N)
        if c.split_k > 1:
            outs["out_f32"][1].copy_(d.get("prev", dev))
    for name, (_, view, _, _) in outs.items():
        kw[name] = view
    if c.fold == "producer":
        n = (N // 128) * M * 2
        flat = torch.full((n + 128,), float("nan"), device=dev)
        outs["row_sums"] = (flat, flat[64:64 + n].view(N // 128, M, 2), None, None)
        kw["row_sums"] = outs["row_sums"][1]
    ops.gemm_nt(a, w, **kw)
    torch.cuda.synchronize()
    return outs


def decode(c, name, view):
    if name == "out_pre" and c.act == G.ACT_GELU_SAVE_GRAD_U8:
        return G.u8_decode(view)
    if name == "out_pre" and c.act == G.ACT_GELU_SAVE_GRAD_E12:
        return G.e12_unpack(view, c.N)
    return view.float()


def run_case(ops, dev, c, seen, kind=None, expect_256=None, given=None):
    if expect_256 is not None:       # a case that moved to the other kernel after a dispatch change must fail here, not test the wrong thing
        assert G.takes_256(c) == expect_256, f"{c.id}: routing mirror says takes_256 = {G.takes_256(c)}"
    if kind is not None:
        assert G.EPI_NAMES[G.epilogue_kind(c)] == kind, f"{c.id}: epilogue_kind mirror gives {G.EPI_NAMES[G.epilogue_kind(c)]}, not {kind}"
    outs = launch(ops, dev, c, given)
    ref = G.reference(c, dev, _ref_cache, given)
    assert set(outs) == set(ref) - {"pre_act"}
    for name, (big, view, rows, width) in outs.items():
        r, s, cls = ref[name]
        if name == "row_sums":
            n = view.numel()
            assert bool(torch.isnan(big[:64]).all() & torch.isnan(big[64 + n:]).all()), f"{c.id} row_sums: a sentinel around the buffer was overwritten"
        else:
            assert_guard_untouched(big, rows, width, f"{c.id} {name}")
        got = decode(c, name, view)
        assert not bool(torch.isnan(got).any()), f"{c.id} {name}: an element inside [0, M) x [0, N) was not written (NaN left)"
        e, idx = G.judge(got, r, s)
        seen[cls] = max(seen.get(cls, 0.0), e)
        print(f"[gemm forms] {c.id} {name} ({cls}): worst e = {e:.4e}, bound {BOUND[cls]:.4e}")
        if not e <= BOUND[cls]:
            if name == "row_sums":
                j, rem = divmod(idx, c.M * 2)
                where = f"slice {j} (columns {128 * j}..+127), row {rem // 2}, {'sum' if rem % 2 == 0 else 'sum of squares'}; {G.locate(c, rem // 2, 128 * j)}"
            else:
                m, n = divmod(idx, c.N)
                where = f"(m, n) = ({m}, {n}): {G.locate(c, m, n)}"
            pytest.fail(f"{c.id} output {name} (class {cls}): worst e = {e:.4e} > bound {BOUND[cls]:.4e} at {where}; "
                        f"got {float(got.flatten()[idx])!r}, ref {float(r.flatten()[idx])!r}, s {float(s.flatten()[idx])!r}")
        if cls == "dg_u8":   # derived, not measured: half a step + what one bf16 ulp of the pre-activation moves gelu' by
            over = (got.double() - r).abs() - G.u8_derived_bound(ref["pre_act"][0])
            assert float(over.max()) <= 0.0, f"{c.id} out_pre: one-byte gelu' off by {float(over.max()):.3e} more than its derived bound"
    return outs


def _ids(cases):
    return [c.id if isinstance(c, G.Case) else f"{c[0]}-{c[1].id}" for c in cases]


# ------------------------------------------------------------------------------------------------ 256x256 kernel
@pytest.mark.parametrize("kind,c", G.cases_256_kinds(), ids=_ids(G.cases_256_kinds()))
def test_256_kinds(ops, dev, seen, kind, c):
    """every instantiated kind x bias x rank-8 update at exactly 128 tiles (M = 7 * 256 + 5, N = 4096), K = 256 (nk = 4) and 384 (nk = 6)"""
    run_case(ops, dev, c, seen, kind, True)


@pytest.mark.parametrize("kind,c", G.cases_256_scaled(), ids=_ids(G.cases_256_scaled()))
def test_256_scaled(ops, dev, seen, kind, c):
    """the GELU forms with pre-activations x 4 (saturated, flushed gelu') and x 0.05 (the linear part)"""
    run_case(ops, dev, c, seen, kind, True)


@pytest.mark.parametrize("kind,c", G.cases_256_strided(), ids=_ids(G.cases_256_strided()))
def test_256_strided(ops, dev, seen, kind, c):
    """every leading dimension wider than its row and no multiple of 64 elements; NaN in every padding column of every operand"""
    run_case(ops, dev, c, seen, kind, True)


def test_256_fold(ops, dev, seen):
    """RES_F32_COPY with row_sums (judged per element too) and ROWNORM_GELU with inputs from ops.ln_fold_weights / ops.rowsum_finalize, judged
    against the folded formula in fp64 and against the un-folded LayerNorm -> Linear -> GELU"""
    (k0, prod), (k1, cons), (_, cons_u) = G.cases_256_fold()
    outs = run_case(ops, dev, prod, seen, k0, True)
    assert torch.equal(_bits(outs["out_bf16"][1]), _bits(outs["out_f32"][1].to(BF16)))          # the copy is the fp32 result's rounding
    del outs
    d = G.draws_for(cons)
    x1, w1 = d.get("x1", dev), d.get("w1", dev)
    M, H = x1.shape
    xs = x1.view(M, H // 128, 128)
    sums = torch.stack([xs.sum(-1).T, (xs * xs).sum(-1).T], dim=-1).contiguous()
    stats = torch.empty((M, 2), device=dev)
    ops.rowsum_finalize(sums, G.LN_EPS, stats)
    wg, s_n, bp = ops.ln_fold_weights(w1, d.get("gamma", dev), d.get("beta", dev), d.get("bias", dev))
    given = dict(wg=wg, s_n=s_n, bp=bp, stats=stats)
    run_case(ops, dev, cons, seen, k1, True, given)
    run_case(ops, dev, cons_u, seen, k1, True, given)


def test_256_tile_order_and_persistent_loop(ops, dev, seen, cus):
    """fewer column tiles than the W-stationary group (N = 768); tiles = CUs + tiles_n or more, from the device's CU count, so some workgroup
    walks a second tile; M = 1024 exactly at N = 8192"""
    cases = G.cases_256_order(cus)
    tiles = -(-cases[2][1].M // 256) * (cases[2][1].N // 256)
    assert tiles >= cus + 4, (tiles, cus)
    for kind, c in cases:
        run_case(ops, dev, c, seen, kind, True)


@pytest.mark.parametrize("pair", range(len(G.threshold_pairs())), ids=["M1023_1024", "tiles127_128"])
def test_threshold_pairs(ops, dev, seen, pair):
    """the same operands on both sides of a routing threshold: each member judged against fp64 in the kernel it lands in"""
    lo, hi = G.threshold_pairs()[pair]
    run_case(ops, dev, hi, seen, None, True)
    run_case(ops, dev, lo, seen, None, False)


# ------------------------------------------------------------------------------------------------ 128x128 kernel
@pytest.mark.parametrize("c", G.cases_128(), ids=_ids(G.cases_128()))
def test_128_epilogue(ops, dev, seen, c):
    """store_row16's branches at ragged N, M in {1, 77, 129, 300}, K in {64, 192}"""
    run_case(ops, dev, c, seen, None, False)


@pytest.mark.parametrize("c", G.cases_128_splitk(), ids=_ids(G.cases_128_splitk()))
def test_128_split_k(ops, dev, seen, c):
    """split_k in {2, 4}: atomic accumulation onto a non-zero fp32 output"""
    run_case(ops, dev, c, seen, None, False)


@pytest.mark.parametrize("c", G.cases_128_hole(), ids=_ids(G.cases_128_hole()))
def test_128_k_hole(ops, dev, seen, c):
    """K hole at the start, middle and end, one tile and K - 64 long, NaN in both operands inside it, against fp64 with the segment removed"""
    run_case(ops, dev, c, seen, None, False)


def test_rejections_launch_nothing(ops, dev):
    """each rejected argument combination of gemm_impl raises, and the outputs still hold their sentinel"""
    M, N, K = 77, 48, 64
    g = torch.Generator().manual_seed(5)
    a = torch.randn(M + 1, K + 8, generator=g).to(dev, BF16)
    w = torch.randn(N, K + 8, generator=g).to(dev, BF16)
    bob, ob = guarded(dev, M, N, N + 8, BF16)
    bof, of = guarded(dev, M, N, N + 4, F32)
    bop, op = guarded(dev, M, N, N + 8, BF16)
    aux, aux8 = torch.randn(M, N + 8, generator=g).to(dev, BF16), torch.zeros((M, N + 8), dtype=U8, device=dev)
    res = torch.randn(M, N + 2, generator=g).to(dev)
    A, W = a[:M, :K], w[:, :K]
    bad = [
        ("K % 64", lambda: ops.gemm_nt(a[:M, :32], w[:, :32], out_bf16=ob)),
        ("N % 16", lambda: ops.gemm_nt(A, W[:40], out_bf16=ob[:, :40])),
        ("lda % 8", lambda: ops.gemm_nt(a.view(-1)[: M * (K + 4)].view(M, K + 4)[:, :K], W, out_bf16=ob)),
        ("misaligned A", lambda: ops.gemm_nt(a.view(-1)[4: 4 + M * (K + 8)].view(M, K + 8)[:, :K], W, out_bf16=ob)),
        ("no output", lambda: ops.gemm_nt(A, W)),
        ("GELU_GRAD without aux", lambda: ops.gemm_nt(A, W, act=ops.ACT_GELU_GRAD, out_bf16=ob)),
        ("MUL_AUX without aux", lambda: ops.gemm_nt(A, W, act=ops.ACT_MUL_AUX, out_bf16=ob)),
        ("ld_aux % 8", lambda: ops.gemm_nt(A, W, act=ops.ACT_ADD_AUX, aux=aux.view(-1)[: M * (N + 4)].view(M, N + 4)[:, :N], out_bf16=ob)),
        ("MUL_AUX_U8 ld_aux % 16", lambda: ops.gemm_nt(A, W, act=ops.ACT_MUL_AUX_U8, aux=aux8[:, :N], out_bf16=ob)),
        ("MUL_AUX_E12 without aux", lambda: ops.gemm_nt(A, W, act=ops.ACT_MUL_AUX_E12, out_bf16=ob)),
        ("SAVE_GRAD without out_pre", lambda: ops.gemm_nt(A, W, act=ops.ACT_GELU_SAVE_GRAD, out_bf16=ob)),
        ("SAVE_GRAD_U8 ld_pre % 16", lambda: ops.gemm_nt(A, W, act=ops.ACT_GELU_SAVE_GRAD_U8, out_pre=aux8[:, :N], out_bf16=ob)),
        ("act out of range", lambda: ops.gemm_nt(A, W, act=10, out_bf16=ob)),
        ("ld_rank_u % 8", lambda: ops.gemm_nt(A, W, rank_u=aux.view(-1)[: M * 12].view(M, 12)[:, :8], rank_v=aux.view(-1)[: N * 8].view(N, 8), out_bf16=ob)),
        ("misaligned bias", lambda: ops.gemm_nt(A, W, bias=res.view(-1)[1: 1 + N], out_bf16=ob)),
        ("ld_res % 4", lambda: ops.gemm_nt(A, W, residual=res[:, :N], out_f32=of)),
        ("ld_out_bf16 % 8", lambda: ops.gemm_nt(A, W, out_bf16=bob.view(-1)[: M * (N + 4)].view(M, N + 4)[:, :N])),
        ("ld_out_f32 % 4", lambda: ops.gemm_nt(A, W, out_f32=bof.view(-1)[: M * (N + 2)].view(M, N + 2)[:, :N])),
        ("ld_pre % 8", lambda: ops.gemm_nt(A, W, out_pre=bop.view(-1)[: M * (N + 4)].view(M, N + 4)[:, :N], out_bf16=ob)),
        ("dropout with split_k", lambda: ops.gemm_nt(A, W, out_f32=of, split_k=2, drop=ops.Drop(0.1, 7))),
        ("split_k with a bf16 output", lambda: ops.gemm_nt(A, W, out_f32=of, out_bf16=ob, split_k=2)),
        ("split_k with an activation", lambda: ops.gemm_nt(A, W, act=ops.ACT_GELU, out_f32=of, split_k=2)),
        ("split_k with a residual", lambda: ops.gemm_nt(A, W, residual=of, out_f32=of, split_k=2)),
        ("hole off the tile grid", lambda: ops.gemm_nt(A, W, out_bf16=ob, k_hole=(32, 32))),
        ("hole past K", lambda: ops.gemm_nt(A, W, out_bf16=ob, k_hole=(64, 64))),
        ("hole covering K", lambda: ops.gemm_nt(A, W, out_bf16=ob, k_hole=(0, 64))),
        ("row_sums outside the 256x256 kernel", lambda: ops.gemm_nt(A, W[:, :K].repeat(3, 1)[:128], bias=torch.zeros(128, device=dev), residual=torch.zeros((M, 128), device=dev),
                                                                   out_f32=torch.full((M, 128), float("nan"), device=dev), out_bf16=torch.full((M, 128), float("nan"), dtype=BF16, device=dev),
                                                                   row_sums=torch.full((1, M, 2), float("nan"), device=dev))),
    ]
    for what, call in bad:
        with pytest.raises(Exception):
            call()
        torch.cuda.synchronize()
        for big, name in ((bob, "out_bf16"), (bof, "out_f32"), (bop, "out_pre")):
            assert_guard_untouched(big, 0, 0, f"rejection '{what}': {name}")        # rows = width = 0: the whole buffer is guard
    # an e4m7 form outside its two 256x256 kinds is declined there (kind -1) and runs on the 128x128 kernel: judged in test_128_epilogue at N = 144;
    # an inconsistent fold epilogue is an error at a 256x256-sized shape too
    big = G.Case(1797, 4096, 256)
    d = G.draws_for(big)
    with pytest.raises(Exception):
        ops.gemm_nt(d.get("A", dev), d.get("W", dev), out_f32=torch.empty((1797, 4096), device=dev), residual=d.get("res", dev),
                    row_sums=torch.empty((32, 1797, 2), device=dev))     # row_sums without bias and the bf16 copy


# ------------------------------------------------------------------------------------------------ split-K workspace paths
def _judge_plain(tag, got, ref_s, seen, shape_n):
    r, s = ref_s
    e, idx = G.judge(got, r, s)
    seen["f32_acc"] = max(seen.get("f32_acc", 0.0), e)
    print(f"[gemm forms] {tag} (f32_acc): worst e = {e:.4e}, bound {BOUND['f32_acc']:.4e}")
    assert e <= BOUND["f32_acc"], (f"{tag}: worst e = {e:.4e} > {BOUND['f32_acc']:.4e} at {divmod(idx, shape_n)} (256x256 tile {tuple(x // 256 for x in divmod(idx, shape_n))}); "
                                   f"got {float(got.flatten()[idx])!r}, ref {float(r.flatten()[idx])!r}")


@pytest.mark.parametrize("M,N,K", G.NT_SPLITK_SHAPES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_nt_splitk(ops, dev, seen, M, N, K, accumulate):
    """gemm_nt_splitk with real-valued operands, accumulate on (onto a non-zero output) and off (over NaN)"""
    assert G.nt_splitk_takes(M, N, K)
    A, W, prev = (t.to(dev) for t in G.nt_splitk_operands(M, N, K))
    A, W = poisoned(A, K + 8), poisoned(W, K + 8)
    big, out = guarded(dev, M, N, N, F32)
    if accumulate:
        out.copy_(prev)
    assert ops.gemm_nt_splitk(A, W, out, accumulate=accumulate) is True
    torch.cuda.synchronize()
    assert_guard_untouched(big, M, N, "nt_splitk out")
    assert not bool(torch.isnan(out).any())
    _judge_plain(f"nt_splitk {M}x{N}x{K} acc={int(accumulate)}", out, G.product(A, W, prev if accumulate else None, True), seen, N)


@pytest.mark.parametrize("M,Na,Nb", G.TN_SPLITK_SHAPES)
@pytest.mark.parametrize("ld_extra", [0, 8])
@pytest.mark.parametrize("colsum,ordered", [(False, False), (True, False), (True, True)])
def test_tn_splitk(ops, dev, seen, M, Na, Nb, ld_extra, colsum, ordered):
    """gemm_tn_splitk with real-valued operands: strided operands, column sums by atomics and in slice order (three runs bit-identical), per element"""
    assert G.tn_splitk_takes(M, Na, Nb)
    A, B, prev, cprev = (t.to(dev) for t in G.tn_splitk_operands(M, Na, Nb))
    A, B = poisoned(A, Na + ld_extra), poisoned(B, Nb + ld_extra)
    runs = []
    for rep in range(3 if ordered else 1):
        big, out = guarded(dev, Na, Nb, Nb, F32)
        accumulate = rep == 0
        if accumulate:
            out.copy_(prev)
        cbig = torch.full((Na + 8,), float("nan"), device=dev)
        cs = cbig[4:4 + Na]
        cs.copy_(cprev)
        assert ops.gemm_tn_splitk(A, B, out, accumulate=accumulate, colsum=cs if colsum else None, ordered=ordered) is True
        torch.cuda.synchronize()
        assert_guard_untouched(big, Na, Nb, "tn_splitk out")
        assert bool(torch.isnan(cbig[:4]).all() & torch.isnan(cbig[4 + Na:]).all())
        assert not bool(torch.isnan(out).any())
        _judge_plain(f"tn_splitk {M}x{Na}x{Nb}+{ld_extra} acc={int(accumulate)}", out, G.product(A.T, B.T, prev if accumulate else None, True), seen, Nb)
        if colsum:
            _judge_plain(f"tn_splitk {M}x{Na}x{Nb}+{ld_extra} colsum ordered={int(ordered)}", cs, G.colsum(A, cprev, True), seen, 1)
        else:
            assert torch.equal(cs, cprev)
        runs.append(cs.clone())
    for r in runs[1:]:
        assert torch.equal(_bits(r), _bits(runs[0]))


def test_splitk_paths_decline_without_writing(ops, dev):
    """shapes outside each path return False and write nothing"""
    g = torch.Generator().manual_seed(9)
    for M, N, K in ((40, 256, 256), (40, 256, 576), (40, 128, 512), (40, 256, 448)):      # nk < 8 | nk odd | N % 256 | K % 128
        assert not G.nt_splitk_takes(M, N, K)
        A, W = torch.randn(M, K, generator=g).to(dev, BF16), torch.randn(N, K, generator=g).to(dev, BF16)
        big, out = guarded(dev, M, N, N, F32)
        assert ops.gemm_nt_splitk(A, W, out) is False
        torch.cuda.synchronize()
        assert_guard_untouched(big, 0, 0, "declined nt_splitk")
    for M, Na, Nb in ((200, 256, 256), (128, 256, 256), (256, 128, 256), (256, 256, 384)):   # M % 128 | M < 256 | Na % 256 | Nb % 256
        assert not G.tn_splitk_takes(M, Na, Nb)
        A, B = torch.randn(M, Na, generator=g).to(dev, BF16), torch.randn(M, Nb, generator=g).to(dev, BF16)
        big, out = guarded(dev, Na, Nb, Nb, F32)
        cs = torch.full((Na,), float("nan"), device=dev)
        assert ops.gemm_tn_splitk(A, B, out, colsum=cs) is False
        torch.cuda.synchronize()
        assert_guard_untouched(big, 0, 0, "declined tn_splitk")
        assert bool(torch.isnan(cs).all())


# ------------------------------------------------------------------------------------------------ transposes and casts
@pytest.mark.parametrize("R,C,ld_in,form", [(77, 50, 50, "general"), (300, 256, 257, "general"), (130, 72, 73, "general"), (300, 256, 256, "fast64"),
                                            (300, 264, 272, "fast64"), (1000, 64, 64, "fast256"), (1500, 128, 136, "fast256")])
def test_transpose_bf16(ops, dev, R, C, ld_in, form):
    """the general form (C % 8 != 0 or an odd ld_in) and both fast forms, R no multiple of the row tile, rows R .. ld_out - 1 zero: exact"""
    Rp = (R + 63) // 64 * 64
    assert G.transpose_form(C, ld_in, Rp) == form
    g = torch.Generator().manual_seed(R + C)
    x = poisoned(torch.randn(R, C, generator=g).to(dev, BF16), ld_in)
    out = ops.transpose_bf16(x)
    torch.cuda.synchronize()
    assert out.shape == (C, Rp)
    assert torch.equal(_bits(out[:, :R]), _bits(x.T.contiguous())) and bool((_bits(out[:, R:]) == 0).all())


@pytest.mark.parametrize("R,C,ld_extra", G.TRANSPOSE_COLSUM_SHAPES)
def test_transpose_colsum(ops, dev, seen, R, C, ld_extra):
    """column sums beside the transpose: with the partials workspace three runs are bit-identical; by atomics (no workspace) judged once"""
    from clibd_amd import _lib

    xh, cprev = G.transpose_operand(R, C, ld_extra)
    xfull = xh.to(dev)
    xfull[:, C:] = float("nan")
    x, cprev = xfull[:, :C], cprev.to(dev)
    want = x.T.contiguous()
    ref = G.colsum(x, cprev, True)
    runs = []
    for _ in range(3):
        cs = cprev.clone()
        out = ops.transpose_bf16(x, colsum=cs)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[:, :R]), _bits(want)) and bool((_bits(out[:, R:]) == 0).all())
        runs.append(cs)
    assert torch.equal(_bits(runs[1]), _bits(runs[0])) and torch.equal(_bits(runs[2]), _bits(runs[0]))
    _judge_plain(f"transpose_colsum {R}x{C}+{ld_extra} workspace", runs[0], ref, seen, 1)
    Rp = (R + 63) // 64 * 64
    out, cs = torch.full((C, Rp), float("nan"), dtype=BF16, device=dev), cprev.clone()
    _lib.check(_lib.load().clibd_transpose_colsum_bf16(x.data_ptr(), x.stride(0), R, C, out.data_ptr(), Rp, cs.data_ptr(), None, 0, ops._stream()), "transpose_colsum_bf16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:, :R]), _bits(want)) and bool((_bits(out[:, R:]) == 0).all())
    _judge_plain(f"transpose_colsum {R}x{C}+{ld_extra} atomics", cs, ref, seen, 1)


def test_transpose_fp8_over_every_byte(ops, dev):
    """every e4m3 byte value at every column phase, scaled by a power of two and by 1 / 1.7: the bf16 rounding of the fp32 product, NaN for NaN"""
    R, C = 100, 264
    codes = ((torch.arange(R)[:, None] * 37 + torch.arange(C + 8)[None, :]) % 256).to(torch.uint8).to(dev)
    x = codes.view(ops.FP8)[:, :C]
    assert len(torch.unique(codes[:, :C])) == 256
    for scale in (0.25, 1.0 / 1.7):
        out = ops.transpose_fp8(x, scale)
        torch.cuda.synchronize()
        want = (x.float() * torch.tensor(scale, dtype=F32, device=dev)).to(BF16).T.contiguous()
        got = out[:, :R]
        nan = torch.isnan(want)
        assert int(nan.sum()) > 0 and torch.equal(torch.isnan(got), nan)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]) and bool((_bits(out[:, R:]) == 0).all())


def test_casts(ops, dev):
    """cast_bf16 at n % 4 in {0, 1, 2, 3} including n < 4 (the tail thread) and past one grid stride; cast_transpose_bf16 at ragged R and C: exact"""
    g = torch.Generator().manual_seed(11)
    for n in (1, 2, 3, 4, 5, 6, 7, 1024, 1025, 4098, 2048 * 256 * 4 + 3):
        x = torch.randn(n, generator=g).to(dev)
        big = torch.full((n + 16,), float("nan"), dtype=BF16, device=dev)
        from clibd_amd import _lib
        _lib.check(_lib.load().clibd_cast_f32_to_bf16(x.data_ptr(), big[8:].data_ptr(), n, ops._stream()), "cast")
        torch.cuda.synchronize()
        assert torch.equal(_bits(big[8:8 + n]), _bits(x.to(BF16))), n
        assert bool(torch.isnan(big[:8]).all() & torch.isnan(big[8 + n:]).all()), n
        assert torch.equal(_bits(ops.cast_bf16(x)), _bits(x.to(BF16)))
    for R, C in ((77, 130), (1, 65), (64, 64), (129, 3)):
        x = torch.randn(R, C, generator=g).to(dev)
        assert torch.equal(_bits(ops.cast_transpose_bf16(x)), _bits(x.to(BF16).T.contiguous())), (R, C)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))       # what tests/conftest.py does for a pytest run
    worst = G.measure_restatement(G.all_epilogue_cases(256), print)
    worst["f32_acc"] = max(worst["f32_acc"], G.measure_splitk(print))
    print("worst e of the restatement against fp64 per class (WORST above; each bound is 3 x):")
    for cls in G.CLASSES:
        print(f"  {cls:13s} {worst[cls]:.4e}   recorded {WORST[cls]:.4e}")
