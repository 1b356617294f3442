"""Every LoRA adapter kernel form of clibd_amd/csrc/lora.hip, per element, against an fp64 statement of the operation from the same bf16 operands.

The operations, the restatement with the kernels' rounding points, the routing mirror, the judgement and the case lists live in
tests/lora_reference.py (CPU-importable).  This module launches every case with sentinels around every output, poison in every operand's
padding (and in the k segment of dqkv, which nothing may read), a byte pattern in every workspace with guard bytes behind it, and gradients
that start from non-zero contents.  Each case asserts the mirror's route before its outputs are judged.

DISPATCH TABLE (read from lora.hip; T = test below)

clibd_lora_pack            rejects null pointer (not expressible through ctypes data_ptr of a live tensor), H <= 0, H % 64           T pack_rejections
                           lora_pack_kernel, grid ceil(3H / 256): H = 64 (one ragged block), 128, 384, 768, 1024                         T pack
clibd_lora_down_proj       rejects M, H <= 0, H % 8, ld_x < H, ld_x % 8, misaligned x / a_cat / t                                         T down_proj_rejections
                           lora_down_proj_kernel, blocks = min(ceil(M / 4), 2048), one wave per row, lanes stride 512 columns:
                           H = 8 (one lane), 128 (lanes 16.. idle), 512 (every lane once), 520 and 768, 1024 (the second trip);
                           M = 1, 3, 4, 5 (ragged block), 8191, 8192 (the cap exactly), 8199 (the grid-stride loop); ld_x = H, H + 8       T down_proj
clibd_lora_workspace_bytes 0 unless M % 32 == 0 and H % 128 == 0; else min(CUs, M / 32) x 16 H floats                                     T ordered_contract
clibd_lora_wgrad           rejects null, M <= 0, H % 64, H > 1024, ld_dqkv < 3H or % 8, ld_dt < 8 or % 8, misaligned dqkv / x / t / dt   T wgrad_backward_rejections
                           MFMA form: M % 32 == 0 and (M >= 8192 or a workspace) and H % 128 == 0 -> lora_wgrad_mfma_kernel<H / 128>
                             (1 .. 8), grid (min((2 CUs + 5) / 6, M / 32), 6), six steps per trip, three slabs in flight                 T mfma, mfma_without_workspace
                             rejects a misaligned or too small workspace                                                                 T ordered_contract
                             with a workspace: partials + lora_reduce_kernel(g, g) (four chains of four + tail)                          T mfma, reduce_chain_tails
                             without: float atomics                                                                                      T mfma_without_workspace
                           otherwise lora_wgrad_kernel, ceil(M / 256) blocks of H threads (a workspace, if passed, is ignored)           T valu, valu_routes
clibd_lora_backward        rejects as wgrad, with ld_dt < 16 and a misaligned w_dt                                                        T wgrad_backward_rejections
                           fused: M % 32 == 0, M >= 131072, H % 256 == 0, 2H / 256 in {4, 6, 8} -> lora_dt_db_kernel<NCH> on min(CUs, M / 32)
                             workgroups, then lora_wgrad_mfma_kernel<H / 128> on the x segments (grid (min((2 CUs + 1) / 2, M / 32), 2)),
                             then lora_reduce_kernel(g_b, g_a) with a workspace; rejects a misaligned or too small workspace              T fused, ordered_contract
                           otherwise clibd_gemm_bf16_nt_khole (N = 16, K = 3H, hole = the k segment) and clibd_lora_wgrad                  T backward_two_call
Out of scope: the LayerNorm-fused down-projection and the GEMM's rank-8 step (test_layernorm_forms_gpu.py, test_gemm_forms_gpu.py); lowering
the fused threshold (not a parameter of the ABI: the fused pair is only ever launched at M >= 131072); the two-call route at M >= 131072 (ragged M, or
H = 128, 256, 384, 640, 896, for which lora_dt_db_kernel has no instantiation) runs the same kernels as T backward_two_call, at a size no test needs;
g_a != g_b in lora_reduce_kernel: both launchers of the fused pair give min(CUs, M / 32) on every CU count ((2 CUs + 1) / 2 == CUs), so the two
halves of a copy always have the same number of writers (the workspace check still treats the halves separately).

JUDGEMENT.  e = |got - ref| / max(|ref|, 2^-10 s) (gemm_reference.judge) for every element of every output; the worst element must meet the bound
of its class: 3 x the worst e of the CPU restatement over this module's real-valued inputs (`python tests/test_lora_forms_gpu.py`, saved as
profiles/lora_forms_cpu_restatement.log; the margin covers the MFMA accumulation order and the order of atomics).  Classes: t; dt by the GEMM; dt by
the fused kernel; gradients by the VALU kernel, by MFMA with atomics, by MFMA with partials.  The integer cases have no bound: every partial sum is
an exact integer, and the four gradients must be bit-equal to the fp64 reference.  The gradients of lora_backward are judged against the fp64
products of the dt the call STORED; that dt is judged against fp64 on its own.  Measured on an MI355X: profiles/lora_forms_mi355x.log."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import lora_reference as L  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8

# worst e of the CPU restatement against fp64 per class (python tests/test_lora_forms_gpu.py; profiles/lora_forms_cpu_restatement.log)
WORST = {"t": 3.8911e-3, "dt_gemm": 3.8899e-3, "dt_fused": 3.8909e-3, "g_valu": 2.8793e-5, "g_mfma_atomic": 1.0003e-5, "g_mfma_partials": 2.1595e-5}
BOUND = {k: 3.0 * v for k, v in WORST.items()}
FILL = 0xA5
FILL_WORD = -1515870811      # 0xA5A5A5A5 as int32
GUARD_BYTES = 256


@pytest.fixture(scope="module")
def ops(dev):
    from clibd_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def lib(dev):
    from clibd_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.fixture(scope="module")
def seen():
    """worst e per class over the module, printed at the end (-s shows it)"""
    w = {}
    yield w
    print("\n[lora forms] worst e per class on this device: " + ", ".join(f"{k} {v:.3e} (bound {BOUND[k]:.3e})" for k, v in sorted(w.items())))


# ------------------------------------------------------------------------------------------------ buffers
def _bits(t):
    return t.view({BF16: torch.int16, F32: torch.int32, U8: torch.uint8}[t.dtype])


def padded(t, ld):
    """operand `t` in a buffer of row stride `ld` whose padding columns are NaN"""
    if ld == t.shape[1]:
        return t.contiguous()
    big = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big


def guarded_rows(dev, rows, width, ld, dtype):
    """an output of rows x width inside a NaN buffer: 3 rows before and after, padding columns up to the stride"""
    big = torch.full((rows + 6, ld), float("nan"), dtype=dtype, device=dev)
    return big, big[3:3 + rows, :width]


def rows_guard_ok(big, rows, width):
    return bool(torch.isnan(big[:3]).all() & torch.isnan(big[3 + rows:]).all() & torch.isnan(big[3:3 + rows, width:]).all())


class Grads:
    """the four gradients, each inside a NaN-guarded flat buffer (64 floats on either side), holding `init`"""

    def __init__(self, dev, H, init):
        self.big, self.view = [], []
        for i0, shape in zip(init, ((4, H), (4, H), (H, 4), (H, 4))):
            b = torch.full((4 * H + 128,), float("nan"), device=dev)
            v = b[64:64 + 4 * H].view(shape)
            v.copy_(i0)
            self.big.append(b)
            self.view.append(v)

    def ptrs(self):
        return [v.data_ptr() for v in self.view]

    def guards_ok(self):
        return all(bool(torch.isnan(b[:64]).all() & torch.isnan(b[-64:]).all()) for b in self.big)

    def unchanged(self, init):
        return all(torch.equal(_bits(v), _bits(i0.to(v.device))) for v, i0 in zip(self.view, init))


class Workspace:
    """`nbytes` of the byte pattern with GUARD_BYTES more behind them"""

    def __init__(self, dev, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + GUARD_BYTES,), FILL, dtype=U8, device=dev)

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what, written_halves, H):
        """written_halves: {(first float, floats)} of every 16 H-float copy expected to be fully written, as (copies, offset, length); everything else keeps the pattern"""
        words = self.buf.view(torch.int32)
        mask = torch.zeros(words.numel(), dtype=torch.bool, device=words.device)
        for copies, off, ln in written_halves:
            m = mask[:copies * 16 * H].view(copies, 16 * H)
            m[:, off:off + ln] = True
        still = words == FILL_WORD
        assert not bool((still & mask).any()), f"{what}: a workspace element of a copy the kernels own still holds the fill pattern (a workgroup did not write its partials)"
        assert bool(still[~mask].all()), f"{what}: workspace bytes outside the copies in use (or the guard bytes behind workspace_bytes) were overwritten"


# ------------------------------------------------------------------------------------------------ one gradient case
_fused_draws = {}


def _operands(c, dev):
    if c.M >= L.FUSED_MIN_M:      # one draw per (H, mode) at the larger M, cut
        key = (c.H, c.mode, c.seed)
        if _fused_draws.get("key") != key:
            _fused_draws.clear()
            torch.cuda.empty_cache()
            _fused_draws.update(key=key, ops=L.operands_for(L.Case(c.entry, L.FUSED_M[1], c.H, True, c.mode, seed=c.seed), dev))
        dqkv, x, t, dt, init, w_dt = _fused_draws["ops"]
        return dqkv[:c.M], x[:c.M], t[:c.M], None, init, w_dt
    return L.operands_for(c, dev)


def _fail_where(c, r, name, idx, cus):
    """the element's place in its kernel, and the rows at which that kernel's loop ends for this M"""
    if r["form"] == "valu":
        m0 = (c.M - 1) // L.LW_ROWS * L.LW_ROWS
        left = c.M - m0
        return (L.locate_valu(name, c.H, idx) + f"; {r['grid'][0][0]} block(s), the last holds rows {m0}..{c.M - 1} ({left} left: {left // 16} whole 16-row trips, "
                f"{left % 16} rows in the clamped tail, last row {c.M - 1} in row group {(c.M - 1) % 4})")
    G = r["grid"][-1 if name.startswith("dA") else 0][0]
    lo, hi = divmod(c.M // 32, G)[0], -(-(c.M // 32) // G)
    return (L.locate_mfma(name, c.H, idx) + f"; {c.M // 32} slabs over {G} workgroups: {lo}|{hi} each, last slab rows {c.M - 32}..{c.M - 1}, "
            f"the last six-step trip of a workgroup runs {(lo - 1) % 6 + 1 if lo else 0}|{(hi - 1) % 6 + 1} steps")


def run_case(ops, lib, dev, cus, c, seen, expect_form):
    r = L.route(c.entry, c.M, c.H, c.workspace, cus)
    assert r["form"] == expect_form, f"{c.id}: the routing mirror sends this case to {r['form']} ({r['kernels']}), the case list means {expect_form}"
    M, H = c.M, c.H
    dqkv, x, t, dt_in, init, w_dt = _operands(c, dev)
    ld = 3 * H + c.ld_extra
    dq_buf = padded(dqkv, ld)
    grads = Grads(dev, H, init)
    need = int(lib.clibd_lora_workspace_bytes(M, H))
    assert need == r["ws_bytes"], f"{c.id}: clibd_lora_workspace_bytes = {need}, mirror {r['ws_bytes']}"
    ws = None
    if c.workspace:
        assert r["form"] == "valu" or need >= r["used_bytes"] > 0, (c.id, need, r["used_bytes"])
        ws = Workspace(dev, need if need else 4096)
    wargs = (ws.ptr(), ws.nbytes) if ws else (None, 0)
    if c.entry == "wgrad":
        dt_buf = padded(dt_in, c.ld_dt)
        code = lib.clibd_lora_wgrad(dq_buf.data_ptr(), ld, x.data_ptr(), t.data_ptr(), dt_buf.data_ptr(), c.ld_dt, M, H, *grads.ptrs(), *wargs, ops._stream())
        dt_used = dt_in
    else:
        ld_dt = max(c.ld_dt, 16)
        dt_big, dt_out = guarded_rows(dev, M, 16, ld_dt, BF16)
        code = lib.clibd_lora_backward(dq_buf.data_ptr(), ld, x.data_ptr(), t.data_ptr(), w_dt.data_ptr(), dt_out.data_ptr(), ld_dt, M, H, *grads.ptrs(), *wargs,
                                       ops._stream())
    torch.cuda.synchronize()
    assert code == 0, f"{c.id}: returned {code}: {lib.clibd_last_error()}"
    assert grads.guards_ok(), f"{c.id}: a sentinel beside a gradient was overwritten"
    if ws:
        if r["form"] == "valu":
            ws.check(c.id, [], H)
        elif r["form"] == "mfma":
            ws.check(c.id, [(r["g_b"], 0, 16 * H)], H)
        else:
            ws.check(c.id, [(r["g_b"], 0, 8 * H), (r["g_a"], 8 * H, 8 * H)], H)
    if c.entry == "backward":
        assert rows_guard_ok(dt_big, M, 16), f"{c.id}: a sentinel around dt was overwritten"
        got = dt_out.float()
        assert not bool(torch.isnan(got).any()), f"{c.id}: a dt element was not written"
        assert bool((_bits(dt_out[:, 8:].contiguous()) == 0).all()), f"{c.id}: dt columns 8..15 are not exact zeros"
        ref, s = L.dt_reference(dqkv, w_dt)
        cls = "dt_fused" if r["form"] == "fused" else "dt_gemm"
        if c.mode == "int":
            bad = torch.nonzero(got.double() != ref)
            assert bad.numel() == 0, f"{c.id} dt (integers): {bad.shape[0]} elements differ, first at {L.locate_rows('dt', int(bad[0, 0]), int(bad[0, 1]), cus, M)}"
        else:
            e, idx = L.judge(got[:, :8], ref[:, :8], s[:, :8])
            seen[cls] = max(seen.get(cls, 0.0), e)
            print(f"[lora forms] {c.id} dt ({cls}): worst e = {e:.4e}, bound {BOUND[cls]:.4e}")
            m, n = divmod(idx, 8)
            assert e <= BOUND[cls], (f"{c.id} dt (class {cls}): worst e = {e:.4e} > bound {BOUND[cls]:.4e} at {L.locate_rows('dt', m, n, cus, M)}; "
                                     f"got {float(got[m, n])!r}, ref {float(ref[m, n])!r}, s {float(s[m, n])!r}")
        dt_used = dt_out.contiguous()
    refs = L.grads_reference(dqkv, x, t, dt_used, init)
    cls = L.grad_class(r, c.workspace)
    for name, got in zip(L.GRADS, grads.view):
        ref, s = refs[name]
        assert not bool(torch.isnan(got).any()), f"{c.id} {name}: NaN (poison was read, or an element was lost)"
        if c.mode == "int":
            bad = torch.nonzero((got.double() != ref).reshape(-1))
            if bad.numel():
                i = int(bad[0])
                pytest.fail(f"{c.id} {name} (integers, must be bit-equal): {bad.shape[0]} elements differ, first at {_fail_where(c, r, name, i, cus)}; "
                            f"got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}")
            continue
        e, idx = L.judge(got, ref, s)
        seen[cls] = max(seen.get(cls, 0.0), e)
        print(f"[lora forms] {c.id} {name} ({cls}): worst e = {e:.4e}, bound {BOUND[cls]:.4e}")
        if not e <= BOUND[cls]:
            pytest.fail(f"{c.id} {name} (class {cls}): worst e = {e:.4e} > bound {BOUND[cls]:.4e} at {_fail_where(c, r, name, idx, cus)}; "
                        f"got {float(got.reshape(-1)[idx])!r}, ref {float(ref.reshape(-1)[idx])!r}, s {float(s.reshape(-1)[idx])!r}")


# ------------------------------------------------------------------------------------------------ lora_pack
@pytest.mark.parametrize("H", L.PACK_H)
def test_pack(ops, dev, H):
    """all four images bit-exact, the zero rows 8..15 and the k segment of w_dt included, inside sentinel-filled buffers"""
    p = L.draw_adapter(H, "real", 9, dev)
    want = L.pack_images(*p)
    bigs, views = [], []
    for shape in ((3 * H, 8), (H, 8), (8, H), (16, 3 * H)):
        n = shape[0] * shape[1]
        b = torch.full((n + 128,), float("nan"), dtype=BF16, device=dev)
        bigs.append(b)
        views.append(b[64:64 + n].view(shape))
    ops.lora_pack(*p, *views)
    torch.cuda.synchronize()
    for name, b, v, w in zip(("v_fwd", "v_bwd", "a_cat", "w_dt"), bigs, views, want):
        assert bool(torch.isnan(b[:64]).all() & torch.isnan(b[-64:]).all()), f"lora_pack {name}: a sentinel was overwritten"
        bad = torch.nonzero(_bits(v.contiguous()) != _bits(w))
        assert bad.numel() == 0, f"lora_pack H = {H}: {name} differs at {bad[0].tolist()} (of {bad.shape[0]} elements)"
    assert bool((_bits(views[3][8:].contiguous()) == 0).all()) and bool((_bits(views[3][:, H:2 * H].contiguous()) == 0).all())


def test_pack_rejections(lib, ops, dev):
    for H in (96, 32, 0, -64):
        Hb = max(abs(H), 64)
        p = [torch.ones((4 * Hb,), device=dev) for _ in range(4)]
        outs = [torch.full((16 * 3 * Hb,), float("nan"), dtype=BF16, device=dev) for _ in range(4)]
        code = lib.clibd_lora_pack(*[t.data_ptr() for t in p], H, *[t.data_ptr() for t in outs], ops._stream())
        torch.cuda.synchronize()
        assert code != 0, f"lora_pack accepted H = {H}"
        assert all(bool(torch.isnan(o).all()) for o in outs), f"lora_pack H = {H}: rejected, yet an output was written"


# ------------------------------------------------------------------------------------------------ lora_down_proj
@pytest.mark.parametrize("H", L.DOWN_H)
def test_down_proj(ops, lib, dev, seen, H):
    """t = bf16(x . a_cat^T) per element at every M of the list, ld_x = H and H + 8 (NaN in the padding)"""
    for M in L.DOWN_M:
        assert L.down_proj_blocks(M) == min((M + 3) // 4, 2048) and (M < 8192 or L.down_proj_blocks(M) == 2048)
        xh, ah = L.draw_down(M, H)
        x, a = xh.to(dev), ah.to(dev)
        ref, s = L.t_reference(x, a)
        for ld in (H, H + 8):
            xb = padded(x, ld)
            big = torch.full((M * 8 + 128,), float("nan"), dtype=BF16, device=dev)
            out = big[64:64 + M * 8].view(M, 8)
            code = lib.clibd_lora_down_proj(xb.data_ptr(), ld, a.data_ptr(), M, H, out.data_ptr(), ops._stream())
            torch.cuda.synchronize()
            assert code == 0, lib.clibd_last_error()
            assert bool(torch.isnan(big[:64]).all() & torch.isnan(big[-64:]).all()), f"down_proj M = {M}, H = {H}, ld = {ld}: a sentinel was overwritten"
            got = out.float()
            assert not bool(torch.isnan(got).any()), f"down_proj M = {M}, H = {H}, ld = {ld}: an element was not written, or the padding was read"
            e, idx = L.judge(got, ref, s)
            seen["t"] = max(seen.get("t", 0.0), e)
            m, n = divmod(idx, 8)
            assert e <= BOUND["t"], (f"down_proj M = {M}, H = {H}, ld_x = {ld}: worst e = {e:.4e} > {BOUND['t']:.4e} at t[{m}, {n}] (block {m // 4 % 2048}, wave {m % 4}, "
                                     f"grid-stride trip {m // 8192}); got {float(got[m, n])!r}, ref {float(ref[m, n])!r}")
        if M == 5:      # the ops wrapper reaches the same kernel
            assert torch.equal(_bits(ops.lora_down_proj(padded(x, H + 8)[:, :H], a)), _bits(out.contiguous()))


def test_down_proj_rejections(lib, ops, dev):
    M, H = 5, 64
    x = torch.ones((M + 1, H + 16), dtype=BF16, device=dev)
    a = torch.ones((9, H), dtype=BF16, device=dev)
    big = torch.full((M * 8 + 16,), float("nan"), dtype=BF16, device=dev)
    t = big[8:8 + M * 8]
    bad = [("H % 8", (x.data_ptr(), H + 8, a.data_ptr(), M, 60, t.data_ptr())), ("ld_x < H", (x.data_ptr(), H - 8, a.data_ptr(), M, H, t.data_ptr())),
           ("ld_x % 8", (x.data_ptr(), H + 4, a.data_ptr(), M, H, t.data_ptr())), ("M = 0", (x.data_ptr(), H, a.data_ptr(), 0, H, t.data_ptr())),
           ("misaligned x", (x.data_ptr() + 2, H + 8, a.data_ptr(), M, H, t.data_ptr())), ("misaligned a_cat", (x.data_ptr(), H + 8, a.data_ptr() + 8, M, H, t.data_ptr())),
           ("misaligned t", (x.data_ptr(), H + 8, a.data_ptr(), M, H, t.data_ptr() + 2))]
    for what, args in bad:
        assert lib.clibd_lora_down_proj(*args, ops._stream()) != 0, f"lora_down_proj accepted {what}"
        torch.cuda.synchronize()
        assert bool(torch.isnan(big).all()), f"lora_down_proj rejected {what}, yet wrote"


# ------------------------------------------------------------------------------------------------ lora_wgrad
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("H", L.VALU_H)
def test_valu(ops, lib, dev, cus, seen, H, mode):
    """lora_wgrad_kernel at every M of the list (1 .. 700: the clamp against m1 - 1 with 1 .. 255 rows left, the 16-row unroll tail, two and three blocks);
    H = 192, 320: a row group straddles a wavefront; H = 1024: 66 176 bytes of LDS; gradients accumulate onto non-zero contents"""
    assert L.valu_lds_bytes(1024) == 66176
    for c in L.cases_valu(H, mode):
        run_case(ops, lib, dev, cus, c, seen, "valu")


@pytest.mark.parametrize("mode", L.MODES)
def test_valu_routes(ops, lib, dev, cus, seen, mode):
    """whole slabs below 8192 without a workspace, ragged M above 8192 (with and without a workspace pointer), H % 128 == 64 with a workspace pointer:
    all VALU, and a workspace that was passed stays untouched"""
    for c in L.cases_valu_routes(mode):
        run_case(ops, lib, dev, cus, c, seen, "valu")


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("H", L.MFMA_H)
def test_mfma(ops, lib, dev, cus, seen, H, mode):
    """lora_wgrad_mfma_kernel<H / 128> with a workspace at slab counts from the device's workgroup count G: 1, 5, G - 1, G, G + 1, 3G + 1, 5G + 1, 6G + 1, 12G + 5"""
    cases = L.cases_mfma(H, mode, cus)
    G = L.wgrad_groups(cus)
    per_wg = {L.route("wgrad", c.M, H, True, cus)["slabs_per_wg"][0] for c in cases}
    if H in (384, 768):
        assert per_wg == {(1, 1), (1, 2), (3, 4), (5, 6), (6, 7), (12, 13)} and G >= 6, (per_wg, G)
        assert [L.route("wgrad", c.M, H, True, cus)["grid"][0][0] for c in cases] == [1, 5, G - 1] + 6 * [G]      # the grid is cut to the slab count
    else:
        assert any(lo != hi and lo > 0 for lo, hi in per_wg)
    for c in cases:
        run_case(ops, lib, dev, cus, c, seen, "mfma")


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("H", L.MFMA_H)
def test_mfma_without_workspace(ops, lib, dev, cus, seen, H, mode):
    """M >= 8192 without a workspace: the MFMA form's float atomics, two slab counts per width"""
    for c in L.cases_mfma_atomic(H, mode, cus):
        run_case(ops, lib, dev, cus, c, seen, "mfma")


@pytest.mark.parametrize("mode", L.MODES)
def test_reduce_chain_tails(ops, lib, dev, cus, seen, mode):
    """lora_reduce_kernel adding G = 2, 3, 4, 13, 16, 17 copies (G = 1, 5 and the device's maximum come from test_mfma; g_a, g_b of the other launcher from test_fused)"""
    for c in L.cases_reduce(mode):
        assert L.route("wgrad", c.M, c.H, True, cus)["g_b"] == c.M // 32
        run_case(ops, lib, dev, cus, c, seen, "mfma")


# ------------------------------------------------------------------------------------------------ lora_backward
def test_backward_two_call(ops, lib, dev, cus, seen):
    """the skinny GEMM with the k hole, then lora_wgrad in whichever form the shape takes: one H per TILES, H = 128 and 256, ragged and whole-slab M"""
    forms = set()
    for c in L.cases_backward_two_call(cus):
        form = L.route("backward", c.M, c.H, c.workspace, cus)["form"]
        assert form == ("mfma" if c.M % 32 == 0 else "valu")
        forms.add((form, c.workspace))
        run_case(ops, lib, dev, cus, c, seen, form)
    assert forms == {("valu", False), ("mfma", True), ("mfma", False)}


@pytest.mark.parametrize("H", L.FUSED_H)
def test_fused(ops, lib, dev, cus, seen, H):
    """lora_dt_db_kernel<NCH> + lora_wgrad_mfma_kernel on the x segments at M = 131072 and 131072 + 32 (operands and the chunked fp64 reference on the device)"""
    for c in L.cases_fused(H):
        r = L.route("backward", c.M, H, c.workspace, cus)
        assert (r["nch"], r["lcm"]) == {512: (4, 4), 768: (6, 12), 1024: (8, 8)}[H]
        run_case(ops, lib, dev, cus, c, seen, "fused")
    _fused_draws.clear()


# ------------------------------------------------------------------------------------------------ contracts
def test_ordered_contract(ops, lib, dev, cus):
    """whenever clibd_lora_workspace_bytes is non-zero and a workspace is passed the route is an MFMA form (never the VALU kernel's atomics); on the
    device ordered=True at H = 128 and 256 either raises or leaves its workspace written; a too small or misaligned workspace is rejected by both entries"""
    from clibd_amd.engine import NotSupportedYet

    for H in range(64, 1025, 64):
        for M in (32, 512, 8192, 700):
            need = int(lib.clibd_lora_workspace_bytes(M, H))
            assert need == L.workspace_bytes(M, H, cus), (M, H, need)
            if need > 0:
                for entry in ("wgrad", "backward"):
                    r = L.route(entry, M, H, True, cus)
                    assert r["form"] in ("mfma", "fused") and 0 < r["used_bytes"] <= need, f"{entry} M = {M}, H = {H}: a workspace of {need} bytes is asked for, the route is {r['form']}"
    for H in (128, 256):
        M = 512
        c = L.Case("backward", M, H, True, "real", seed=10)
        dqkv, x, t, _, init, w_dt = L.operands_for(c, dev)
        dqkv = torch.nan_to_num(dqkv, nan=0.0)
        grads = [i0.clone() for i0 in init]
        dt = torch.empty((M, 16), dtype=BF16, device=dev)
        ws = Workspace(dev, int(lib.clibd_lora_workspace_bytes(M, H)))
        try:
            ops.lora_backward(dqkv, x, t, w_dt, dt, *grads, workspace=ws.buf[:ws.nbytes], ordered=True)
        except NotSupportedYet:
            continue
        torch.cuda.synchronize()
        g = L.route("backward", M, H, True, cus)["g_b"]
        ws.check(f"ordered lora_backward M = {M}, H = {H}", [(g, 0, 16 * H)], H)
    # workspace rejections, both entries (wgrad in its MFMA form, backward in its fused form)
    for entry, M, H in (("wgrad", 64, 384), ("backward", L.FUSED_MIN_M, 512)):
        c = L.Case(entry, M, H, True, "int", seed=10)
        dqkv, x, t, dt_in, init, w_dt = L.operands_for(c, dev)
        need = int(lib.clibd_lora_workspace_bytes(M, H))
        ws = Workspace(dev, need)
        for what, wargs in (("too small", (ws.ptr(), L.route(entry, M, H, True, cus)["used_bytes"] - 4)), ("misaligned", (ws.ptr() + 4, need))):
            grads = Grads(dev, H, init)
            if entry == "wgrad":
                code = lib.clibd_lora_wgrad(dqkv.data_ptr(), 3 * H, x.data_ptr(), t.data_ptr(), dt_in.data_ptr(), 8, M, H, *grads.ptrs(), *wargs, ops._stream())
            else:
                dt_big, dt_out = guarded_rows(dev, M, 16, 16, BF16)
                code = lib.clibd_lora_backward(dqkv.data_ptr(), 3 * H, x.data_ptr(), t.data_ptr(), w_dt.data_ptr(), dt_out.data_ptr(), 16, M, H, *grads.ptrs(), *wargs, ops._stream())
            torch.cuda.synchronize()
            assert code != 0, f"{entry} accepted a {what} workspace"
            assert grads.unchanged(init) and grads.guards_ok(), f"{entry} rejected a {what} workspace, yet changed a gradient"
            ws.check(f"{entry} with a {what} workspace", [], H)
            if entry == "backward":
                assert bool(torch.isnan(dt_big).all()), "lora_backward rejected its workspace, yet wrote dt"


def test_wgrad_backward_rejections(lib, ops, dev):
    """every rejected argument of clibd_lora_wgrad / clibd_lora_backward returns an error and leaves gradients, dt and sentinels as they were"""
    M, H = 64, 128
    c = L.Case("wgrad", M, H, False, "int", seed=11)
    dqkv, x, t, dt_in, init, _ = L.operands_for(c, dev)
    w_dt = L.pack_images(*L.draw_adapter(H, "int", 11, dev))[3]
    dq_buf = padded(dqkv, 3 * H + 16)
    dt_buf = padded(dt_in, 32)
    wide = [torch.randn(s, device=dev) for s in ((4, 1088), (4, 1088), (1088, 4), (1088, 4))]
    P = dict(dqkv=dq_buf.data_ptr(), ld=3 * H + 16, x=x.data_ptr(), t=t.data_ptr(), dt=dt_buf.data_ptr(), ld_dt=32, M=M, H=H, w_dt=w_dt.data_ptr())
    common = [("H % 64", dict(H=96)), ("H > 1024", dict(H=1088)), ("M = 0", dict(M=0)), ("ld_dqkv < 3H", dict(ld=3 * H - 8)), ("ld_dqkv % 8", dict(ld=3 * H + 4)),
              ("ld_dt % 8", dict(ld_dt=20)), ("misaligned dqkv", dict(dqkv=P["dqkv"] + 2)), ("misaligned x", dict(x=P["x"] + 8)), ("misaligned t", dict(t=P["t"] + 4)),
              ("misaligned dt", dict(dt=P["dt"] + 2))]
    for entry, extra in (("wgrad", [("ld_dt < 8", dict(ld_dt=0))]), ("backward", [("ld_dt < 16", dict(ld_dt=8)), ("misaligned w_dt", dict(w_dt=P["w_dt"] + 2))])):
        for what, change in common + extra:
            a = dict(P, **change)
            g = Grads(dev, 1088, wide) if a["H"] > 1024 else Grads(dev, H, init)
            dt_big, dt_out = guarded_rows(dev, M, 16, 32, BF16)
            if entry == "wgrad":
                code = lib.clibd_lora_wgrad(a["dqkv"], a["ld"], a["x"], a["t"], a["dt"], a["ld_dt"], a["M"], a["H"], *g.ptrs(), None, 0, ops._stream())
            else:
                dtp = dt_out.data_ptr() + (a["dt"] - P["dt"])
                code = lib.clibd_lora_backward(a["dqkv"], a["ld"], a["x"], a["t"], a["w_dt"], dtp, a["ld_dt"], a["M"], a["H"], *g.ptrs(), None, 0, ops._stream())
            torch.cuda.synchronize()
            assert code != 0, f"lora_{entry} accepted {what}"
            assert g.unchanged(wide if a["H"] > 1024 else init) and g.guards_ok(), f"lora_{entry} rejected {what}, yet changed a gradient"
            assert bool(torch.isnan(dt_big).all()), f"lora_{entry} rejected {what}, yet wrote dt"


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))       # what tests/conftest.py does for a pytest run
    fused = "--fused" in sys.argv
    worst = L.measure_restatement(L.all_gradient_cases(256, fused=fused), 256, print)
    worst["t"] = L.measure_down_proj(print)
    print("worst e of the restatement against fp64 per class (WORST above; each bound is 3 x):")
    for cls in L.CLASSES:
        print(f"  {cls:16s} {worst[cls]:.4e}   recorded {WORST[cls]:.4e}")
