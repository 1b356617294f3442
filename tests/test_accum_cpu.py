"""CPU checks of gradient accumulation (clibd_amd.optim, clibd_amd.mlm, include/clibd_hip_accum.h): the fourteenth header and its binding
table, every host refusal of clibd_grad_norm_div, the unit's resource report, the window state machine of the optimizer with the launches
stubbed, the drivers' refusals, the seed rule, the restatements of tests/accum_reference.py, and the documents."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import accum_reference as AR  # noqa: E402
import optim_reference as OR  # noqa: E402

HEADER = ROOT / "include" / "clibd_hip_accum.h"
SYMBOLS = ["clibd_grad_norm_div", "clibd_grad_norm_div_workspace_bytes"]
KERNELS = ["grad_sumsq_div_kernel", "grad_norm_div_finish_kernel"]


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


# ---- header, binding, build -------------------------------------------------------------------------------------------------------------
def test_accum_header_symbols_opening_comment_and_one_pass1_source():
    from clibd_amd import _lib, build

    assert sorted(_lib.HEADERS[HEADER.name]) == SYMBOLS
    assert sorted(_lib.HEADERS["clibd_hip_optim.h"]) == ["clibd_adam_l2_step_groups", "clibd_adamw_step_groups", "clibd_grad_norm", "clibd_grad_norm_workspace_bytes"]
    opening = HEADER.read_text().split("*/")[0]
    assert "stays 7" in opening and "purely additive" in opening and "no float atomic" in opening and "fourteenth" in opening
    assert "accum" in build.SOURCES and build.SOURCES[-1] == "rollout" and HEADER in build._deps()
    assert (build.CSRC / "grad_norm_pass1.h") in build._deps()
    # pass 1 has ONE source: both units include it and neither restates the accumulation loop
    for unit in ("optim.hip", "accum.hip"):
        src = (build.CSRC / unit).read_text()
        assert '#include "grad_norm_pass1.h"' in src and "grad_sumsq_chunk(" in src and "fmaf(x.x, x.x, acc)" not in src
    assert "fmaf(x.x, x.x, acc)" in (build.CSRC / "grad_norm_pass1.h").read_text()


def test_accum_unit_uses_no_scratch():
    """the compiler's resource remark for every kernel of accum.hip: two kernels, no scratch"""
    from clibd_amd import build

    out = [(k["name"], k["scratch"]) for k in build.resource_usage("accum")]
    assert len(out) == len(KERNELS) and all(any(k in n for n, _ in out) for k in KERNELS), out
    assert not [(n, s) for n, s in out if s != 0], out


def test_host_validation_needs_no_gpu(lib):
    """every refusal happens before any launch: the device pointers below are never dereferenced"""
    from clibd_amd import _lib

    L = _lib.load()
    P = ctypes.c_void_p
    a, r, w, d = P(1 << 12), P(1 << 20), P(1 << 24), P(1 << 26)
    ws_of = L.clibd_grad_norm_div_workspace_bytes
    for n in (0, 1, 64 * OR.CHUNK, 64 * OR.CHUNK + 1, 257 * OR.CHUNK + 3):
        assert ws_of(n) == L.clibd_grad_norm_workspace_bytes(n)
    assert ws_of(0) == 256 and ws_of(64 * OR.CHUNK + 1) == 512

    def norm(g=a, n=100000, gs=1.0, mx=1.0, skip=0, div=d, rec=r, ws=w, ws_bytes=256):
        return L.clibd_grad_norm_div(g, n, gs, mx, skip, div, rec, ws, ws_bytes, None)

    cases = [(dict(g=None), b"null"), (dict(rec=None), b"null"), (dict(ws=None, ws_bytes=0), b"null"),
             (dict(ws=None), b"workspace size without a workspace"), (dict(ws=P((1 << 24) + 8)), b"too small or misaligned"),
             (dict(ws_bytes=0), b"too small or misaligned"), (dict(n=65 * OR.CHUNK), b"clibd_grad_norm_div_workspace_bytes"),
             (dict(mx=-1.0), b"max_norm"), (dict(mx=float("nan")), b"max_norm"), (dict(g=P((1 << 12) + 4)), b"misaligned"),
             (dict(rec=P((1 << 20) + 2)), b"misaligned"), (dict(div=P((1 << 26) + 2)), b"misaligned"), (dict(div=P((1 << 26) + 1)), b"misaligned")]
    for kw, word in cases:
        assert norm(**kw) == -1, kw
        msg = L.clibd_last_error()
        assert msg.startswith(b"grad_norm_div:") and word in msg, (kw, msg)
    assert norm(n=0) == 0 and norm(n=0, mx=0.0, skip=1, div=None) == 0           # nothing to do, nothing launched; a NULL divisor is allowed


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------
def test_divisor_rule_and_restatements():
    assert [float(AR.divisor_of(x)) for x in AR.DIVISORS] == [1.0, 1.0, 7.0, float(2 ** 20 + 3), 1.0]
    assert float(AR.divisor_of(-5.0)) == 1.0 and float(AR.divisor_of(float("nan"))) == 1.0 and float(AR.divisor_of(0.5)) == 1.0
    assert AR.SIZES == [1, 3, 16384, 16385, 3 * 16384 + 5]
    for n in AR.SIZES:
        g = OR.gradient(n)
        for div in AR.DIVISORS:
            ref, gate, err32 = AR.norm_div_gate(g, 0.25, div)
            assert ref > 0 and err32 < 1e-6 and OR.NORM_FLOOR <= gate < 3e-6, (n, div, err32)
            if float(AR.divisor_of(div)) == 1.0:          # no divisor: optim_reference's numbers, bit for bit
                assert AR.norm_div_fp32_kernel_order(g, 0.25, div) == OR.norm_fp32_kernel_order(g, 0.25) and ref == OR.norm_fp64(g, 0.25)
    assert float(AR.coef_div(np.float32(4.0), 1.0, 7.0)) == float(np.float32(np.float32(1.0) / (np.float32(4.0) + np.float32(1e-6))) / np.float32(7.0))
    assert float(AR.coef_div(np.float32(0.5), 1.0, 7.0)) == float(np.float32(1.0) / np.float32(7.0)) and float(AR.coef_div(np.float32(9.0), None, None)) == 1.0


# ---- the optimizer's window state machine, launches stubbed ---------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    """FusedAdamW / FusedAdam over CPU tensors: the device check and every launch replaced by a recorder"""
    from clibd_amd import ops, optim

    calls = []
    monkeypatch.setattr(optim.FusedAdamW, "_check_params", staticmethod(lambda ps, dev: None))
    monkeypatch.setattr(ops, "grad_norm_workspace", lambda n, dev: torch.zeros(256, dtype=torch.uint8))
    for name in ("adamw_step", "adam_l2_step", "adamw_step_groups", "adam_l2_step_groups", "grad_norm", "grad_norm_div"):
        monkeypatch.setattr(ops, name, (lambda nm: lambda *a, **k: calls.append((nm, a)))(name))
    return calls


def _params(n=2):
    return [torch.nn.Parameter(torch.ones(70)) for _ in range(n)]


@pytest.mark.parametrize("kind", ["adamw", "adam_l2"])
def test_window_state_machine(stubbed, kind):
    from clibd_amd.optim import FusedAdam, FusedAdamW

    cls, plain = (FusedAdamW, "adamw_step") if kind == "adamw" else (FusedAdam, "adam_l2_step")
    opt = cls(_params(), lr=1e-3, accumulation_steps=3)
    opt.grad_scale = 0.5
    assert opt.accumulation_steps == 3 and opt.divisor_slot is None and not opt.window_open and not opt.window_closes and opt.micro_steps == 0
    for window in range(2):
        for micro in range(3):
            opt.zero_grad()
            if micro == 0:
                assert float(opt.flat_comm.abs().max()) == 0.0                  # a window opens: the bucket and aux are cleared
            else:
                assert float(opt.flat_g.min()) == float(micro) and float(opt.aux[5]) == float(micro)   # inside a window they are kept
            opt.flat_g.add_(1.0)
            opt.aux[5] += 1.0
            assert opt.window_closes == (micro == 2)
            opt.step()
            assert opt.window_open == (micro < 2) and opt.step_count == window + (micro == 2) and len(stubbed) == window + (micro == 2)
    # the k-th call is the plain single launch with grad_scale / micro-steps, the step counted once per window
    assert [c[0] for c in stubbed] == [plain, plain]
    assert stubbed[0][1][9] == 1 and stubbed[1][1][9] == 2 and stubbed[0][1][10] == 0.5 / 3
    # flush: a partial window of two; none open: no launch
    del stubbed[:]
    opt.zero_grad(); opt.step(); opt.zero_grad(); opt.step()
    assert opt.window_open and opt.micro_steps == 2 and not stubbed
    assert opt.flush() is True and not opt.window_open and opt.step_count == 3 and stubbed[0][1][10] == 0.5 / 2
    assert opt.flush() is False and len(stubbed) == 1 and opt.step_count == 3
    opt.zero_grad()
    assert float(opt.flat_comm.abs().max()) == 0.0


def test_window_with_clipping_groups_and_the_device_divisor(stubbed):
    from clibd_amd.optim import FusedAdamW

    a, b = _params(1), _params(1)
    opt = FusedAdamW([{"params": a, "lr": 1e-3}, {"params": b, "lr": 2e-3, "weight_decay": 0.0}], max_grad_norm=1.0, nonfinite="skip",
                     accumulation_steps=2)
    opt.zero_grad(); opt.step()
    assert not stubbed
    opt.zero_grad(); opt.step()
    assert [c[0] for c in stubbed] == ["grad_norm", "adamw_step_groups"]
    norm, upd = stubbed[0][1], stubbed[1][1]
    assert norm[3] == 0.5 and norm[4] == 1.0 and norm[5] is True and upd[9] == 0.5 and upd[10] is opt._record and upd[8] == 1
    # the device divisor: grad_norm_div on aux[slot], grad_scale untouched by the micro-step count, always the grouped update
    del stubbed[:]
    one = FusedAdamW(_params(), lr=1e-3, accumulation_steps=2)
    one.divisor_slot = 1
    one.zero_grad(); one.step(); one.zero_grad(); one.step()
    assert [c[0] for c in stubbed] == ["grad_norm_div", "adamw_step_groups"]
    div, upd = stubbed[0][1], stubbed[1][1]
    assert div[3].data_ptr() == one.aux[1:2].data_ptr() and div[3].numel() == 1 and div[4] == 1.0 and div[5] is None and div[6] is False
    assert upd[9] == 1.0 and upd[10] is one._record
    one.divisor_slot = 64
    one.zero_grad(); one.step(); one.zero_grad()
    with pytest.raises(ValueError, match="divisor_slot"):
        one.step()


def test_k_1_launches_what_it_launched(stubbed):
    """accumulation_steps=1, no divisor slot: every step clears the bucket and is the single plain launch with grad_scale itself"""
    from clibd_amd.optim import FusedAdamW

    opt = FusedAdamW(_params(), lr=1e-3)
    opt.grad_scale = 1.0 / 3
    for i in range(3):
        opt.flat_g.add_(1.0)
        assert opt.window_closes and not opt.window_open
        opt.step()
        assert stubbed[-1][0] == "adamw_step" and stubbed[-1][1][10] == 1.0 / 3 and stubbed[-1][1][9] == i + 1 and len(stubbed) == i + 1
        opt.zero_grad()
        assert float(opt.flat_comm.abs().max()) == 0.0
    assert opt.flush() is False


def test_refusals(stubbed, tmp_path):
    from clibd_amd import checkpoint, mlm, optim
    from clibd_amd.optim import FusedAdam, FusedAdamW

    for cls in (FusedAdamW, FusedAdam):
        for bad in (0, -1, 1.5, True, None):
            with pytest.raises(ValueError, match="accumulation_steps"):
                cls(_params(), accumulation_steps=bad)
    opt = FusedAdamW(_params(), lr=1e-3, accumulation_steps=2)
    model = torch.nn.Linear(2, 2)
    opt.zero_grad(); opt.step()
    with pytest.raises(ValueError, match="middle of an accumulation window"):
        checkpoint.save_training_state(str(tmp_path / "s.pt"), model, opt)
    assert not (tmp_path / "s.pt").exists()
    # drivers that all-reduce the bucket at every step refuse windows under data parallel
    with pytest.raises(ValueError, match="reduced twice"):
        optim.refuse_windows_under_data_parallel(opt, "SimCLR")
    optim.refuse_windows_under_data_parallel(FusedAdamW(_params()), "SimCLR")
    optim.refuse_windows_under_data_parallel(torch.optim.SGD(_params(), lr=0.1), "SimCLR")
    assert 'refuse_windows_under_data_parallel(self.optimizer, "SimCLR")' in (ROOT / "clibd_amd" / "simclr.py").read_text()
    assert 'refuse_windows_under_data_parallel(self.optimizer, "Trainer")' in (ROOT / "clibd_amd" / "train.py").read_text()
    # the masked-LM window needs the flat bucket, and k cannot change in the middle of a window
    with pytest.raises(mlm.NotSupportedYet, match="flat"):
        mlm._window_of(torch.optim.SGD(_params(), lr=0.1), 2, 1, "pretrain_step")
    with pytest.raises(ValueError, match="middle"):
        mlm._window_of(opt, 4, 1, "pretrain_step")
    with pytest.raises(ValueError, match=">= 1"):
        mlm._window_of(opt, 0, 1, "pretrain_step")
    assert mlm._window_of(opt, None, 1, "x") == (2, True) and mlm._window_of(FusedAdamW(_params()), None, 2, "x") == (1, True)
    assert mlm._window_of(torch.optim.SGD(_params(), lr=0.1), None, 1, "x") == (1, False)
    fresh = FusedAdamW(_params())
    assert mlm._window_of(fresh, 4, 1, "x") == (4, True) and fresh.accumulation_steps == 4


def test_micro_seeds_differ_between_ranks_and_micro_steps():
    from clibd_amd import mlm

    seeds = {mlm.micro_seed(s, r, m) for s in (0, 1, 12345) for r in range(8) for m in range(64)}
    assert len(seeds) == 3 * 8 * 64 and all(0 <= x < 2 ** 31 for x in seeds)
    assert mlm.micro_seed(7, 1, 0) != mlm.micro_seed(7, 0, 1) and mlm.micro_seed(7, 2, 3) == mlm.micro_seed(7, 2, 3)
    assert (mlm.AUX_COUNT, mlm.AUX_LOSS, mlm.AUX_HITS) == (1, 2, 3)


# ---- documents -----------------------------------------------------------------------------------------------------------------------------
def test_documents_and_docstrings():
    from clibd_amd import mlm, optim, simclr, train

    for word in ("accumulation_steps", "window_closes", "flush()", "divisor_slot", "mean of the micro-batches' mean", "2^24", "reduced twice",
                 "contrastive", "save_training_state", "§3.18"):
        assert word in optim.__doc__, word
    for word in ("accumulation_steps", "world_size", "sum mode", "GLOBAL labelled count", "num_items_in_batch", "mean of per-rank means", "2^24",
                 "all_reduce", "DistributedSampler", "micro_seed", "flush", "evaluate", "unmeasured", "§3.18"):
        assert word in mlm.__doc__, word
    assert "negatives" in train.Trainer.__init__.__doc__ and "accumulation_steps" in train.Trainer.__init__.__doc__
    assert "accumulation_steps" in simclr.SimCLR.__doc__
    design = (ROOT / "DESIGN.md").read_text()
    assert design.index("### 3.17") < design.index("### 3.18") < design.index("## 4. Oracle")
    sec = design[design.index("### 3.18"):]
    for word in ("accum.hip", "clibd_hip_accum.h", "grad_norm_pass1.h", "clibd_grad_norm_div", "divisor", "VGPR", "scratch", "Occupancy", "2^24",
                 "num_items_in_batch", "mean of per-rank means", "measured", "profiles/accum.log", "bench_accum.py", "unmeasured", "evaluate",
                 "contrastive"):
        assert word in sec, word
    assert "accumulation_steps" in (ROOT / "README.md").read_text() and "accumulation_steps" in (ROOT / "INTEGRATION.md").read_text()
    assert (ROOT / "tools" / "bench_accum.py").exists() and (ROOT / "profiles" / "accum.log").exists()
