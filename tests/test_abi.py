"""CPU checks of the drop-in boundary: the C-ABI library builds, loads, and exports exactly what the headers under include/ declare, with
the types they declare (no compute calls here: there is no GPU on the authoring box)."""
import ctypes
import re
from pathlib import Path

import pytest

from tests import header_reference as HR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "clibd_hip.h"
# how many functions each header declares: a new header adds its key to clibd_amd._lib.HEADERS and its count here, and needs no test of its own
SYMBOL_COUNTS = {"clibd_hip.h": 74, "clibd_hip_accum.h": 2, "clibd_hip_analysis.h": 4, "clibd_hip_attn_wide.h": 2, "clibd_hip_classifier.h": 7,
                 "clibd_hip_insect.h": 3, "clibd_hip_jpeg.h": 3, "clibd_hip_mlm.h": 4, "clibd_hip_mlm_labels.h": 3, "clibd_hip_mlp.h": 3,
                 "clibd_hip_optim.h": 4, "clibd_hip_rollout.h": 4, "clibd_hip_simclr.h": 4, "clibd_hip_views.h": 2}


def declared_symbols():
    return HR.mentioned_symbols(HEADER)


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


def test_header_declares_expected_entry_points():
    syms = declared_symbols()
    for must in ("clibd_gemm_bf16_nt", "clibd_layernorm_fwd", "clibd_attention_fwd", "clibd_attention_bwd", "clibd_lora_wgrad",
                 "clibd_softce_rows_fwd", "clibd_softce_rows_bwd", "clibd_l2norm_fwd", "clibd_adamw_step"):
        assert must in syms


def test_library_exports_every_declared_symbol(lib):
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"declared in clibd_hip.h but not exported: {missing}"


def test_python_binding_covers_every_declared_symbol(lib):
    from clibd_amd import _lib

    assert sorted(_lib.HEADERS["clibd_hip.h"]) == declared_symbols() and len(_lib.HEADERS["clibd_hip.h"]) == 74
    assert _lib.load().clibd_abi_version() == _lib.ABI_VERSION == 7


@pytest.mark.parametrize("header", HR.headers(), ids=lambda h: h.name)
def test_header_and_binding_agree_by_type(lib, header):
    """Every prototype of every header against clibd_amd._lib.HEADERS: the names, the return type, the number of arguments and each
    argument's type as read from the header's text (tests/header_reference.py), and the loaded function carries them."""
    from clibd_amd import _lib

    protos, table = HR.prototypes(header), _lib.HEADERS[header.name]
    assert sorted(protos) == HR.mentioned_symbols(header)       # a `clibd_*(` the prototype reader did not take for a prototype
    assert sorted(protos) == sorted(table)
    assert len(protos) == SYMBOL_COUNTS[header.name]
    assert not [s for s in protos if not hasattr(lib, s)]
    L = _lib.load()
    for name, (res, args) in protos.items():
        assert table[name][0] is res, f"{name}: {header.name} returns {res.__name__}, the binding {table[name][0].__name__}"
        assert [a.__name__ for a in table[name][1]] == [a.__name__ for a in args], f"{name}: argument types differ from {header.name}"
        assert table[name][1] == args, name
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_one_table_covers_the_headers_on_disk():
    from clibd_amd import _lib

    assert set(_lib.HEADERS) == {h.name for h in HR.headers()} == set(SYMBOL_COUNTS)
    assert len(_lib.SIGNATURES) == 119 == sum(SYMBOL_COUNTS.values())       # no symbol sits under two headers
    assert _lib.SIGNATURES == {s: sig for table in _lib.HEADERS.values() for s, sig in table.items()}
    with pytest.raises(ValueError, match="two headers"):
        _lib._flatten({"a.h": {"clibd_x": (ctypes.c_int, [])}, "b.h": {"clibd_x": (ctypes.c_int, [])}})
    assert _lib.load().clibd_abi_version() == _lib.ABI_VERSION == 7


@pytest.mark.parametrize("header", HR.headers(), ids=lambda h: h.name)
def test_source_hash_covers_every_header(header, monkeypatch, tmp_path):
    """csrc_hash() — what clibd_build_hash() bakes in and load() compares — moves with the text of each public header, and every unit depends on it."""
    from clibd_amd import build

    before = build.csrc_hash()
    inc = tmp_path / "include"
    inc.mkdir()
    for h in HR.headers():
        (inc / h.name).write_text(h.read_text() + ("\n/* changed */\n" if h == header else ""))
    monkeypatch.setattr(build, "INCLUDE", inc)
    assert build.csrc_hash() != before
    assert inc / header.name in build._deps()
    monkeypatch.undo()
    assert build.csrc_hash() == before and header in build._deps()


def test_binding_refuses_a_library_built_from_other_sources(lib, monkeypatch):
    """clibd_build_hash() (baked in by clibd_amd/build.py) must equal the hash of the sources beside the library."""
    from clibd_amd import _lib, build

    L = _lib.load()
    assert L.clibd_build_hash().decode() == build.csrc_hash()
    monkeypatch.setattr(build, "csrc_hash", lambda: "0123456789abcdef")
    with pytest.raises(_lib.ClibdHipError, match="built from other kernel sources"):
        _lib._check_build_hash(L)


def test_epilogue_struct_layout_matches_header():
    from clibd_amd._lib import GemmEpilogue, OptimGroup

    # 8 pointers + 8 int32 + 4 dropout words + (ABI 3) the three LN-fold pointers: 8*8 + 12*4 + 3*8 = 136 bytes
    assert ctypes.sizeof(GemmEpilogue) == 136
    # field names, their order and each field's type, as the headers declare them
    assert GemmEpilogue._fields_ == HR.struct_fields(HEADER, "clibd_gemm_epilogue") and len(GemmEpilogue._fields_) == 23
    assert OptimGroup._fields_ == HR.struct_fields(ROOT / "include" / "clibd_hip_optim.h", "clibd_optim_group") and ctypes.sizeof(OptimGroup) == 16


def test_host_side_validation_needs_no_gpu(lib):
    """Bad shapes are rejected on the host before any launch."""
    from clibd_amd import _lib

    L = _lib.load()
    ep = _lib.GemmEpilogue()
    assert L.clibd_gemm_bf16_nt(None, 64, None, 64, 8, 16, 64, ctypes.byref(ep), None, 0, None) == -1
    assert b"null" in L.clibd_last_error()
    assert L.clibd_attention_fwd(ctypes.c_void_p(16), 1, 300, 1, None, ctypes.c_void_p(16), 300, 300, 0, 0, 1.0, 0.0, None, None, None) == -1
    assert L.clibd_softce_workspace_bytes(32, 32, 768) > 32 * 32 * 4
    # round 6: the stream-K tail plan (256 CUs assumed without a device): 591 tiles = 2 rounds + 79 -> 3 K-slices; 399 tiles (tail 143) and K = 768: none
    assert L.clibd_gemm_tail_workspace_bytes(50432, 768, 3072) == 1024 + 79 * 2 * 256 * 256 * 4
    assert L.clibd_gemm_tail_workspace_bytes(50432, 768, 2304) == 1024 + 79 * 2 * 256 * 256 * 4
    assert L.clibd_gemm_tail_workspace_bytes(34048, 768, 3072) == 0 and L.clibd_gemm_tail_workspace_bytes(50432, 3072, 768) == 0
    assert L.clibd_gemm_tail_workspace_bytes(403456, 768, 3072) == 1024 + 120 * 1 * 256 * 256 * 4      # the metric's batch: 4 728 tiles = 18 rounds + 120 -> 2 slices
    assert L.clibd_gemm_tail_workspace_bytes(403456, 768, 3072) <= 48 * 1024 * 1024 + 1024


def test_layernorm_and_attention_argument_combinations_are_validated_on_the_host(lib):
    """The optional arguments of the one-entry-point-per-operation forms: every inconsistent combination is rejected before a launch."""
    from clibd_amd import _lib

    L = _lib.load()
    p = ctypes.c_void_p(256)   # never dereferenced
    ws = L.clibd_layernorm_bwd_pg_workspace_bytes(64, 768)

    def ln_bwd(dres_f32=None, dres_bf16=None, dx_f32=None, dx_res=None, dx_bf16=None, dx_fp8=None, row_dequant=None, dgamma=None, dbeta=None,
               workspace=None, workspace_bytes=0):
        return L.clibd_layernorm_bwd(p, None, p, p, p, 64, 768, dres_f32, dres_bf16, dx_f32, dx_res, dx_bf16, 0, 0, 1.0, dx_fp8, row_dequant,
                                     dgamma, dbeta, workspace, workspace_bytes, None)

    assert ln_bwd(dx_bf16=p, dx_fp8=p) == -1 and b"row_dequant" in L.clibd_last_error()
    assert ln_bwd(dx_bf16=p, dgamma=p) == -1 and b"dbeta" in L.clibd_last_error()
    assert ln_bwd(dx_bf16=p, dres_f32=p, dres_bf16=p) == -1 and b"either fp32 or bf16" in L.clibd_last_error()
    assert ln_bwd(dx_bf16=p, workspace=p, workspace_bytes=ws) == -1 and b"workspace" in L.clibd_last_error()
    assert ln_bwd() == -1 and b"no output" in L.clibd_last_error()

    def ln_fwd(y_bf16=None, lora_a=None, t=None, y_fp8=None, fp8_scale=0.0):
        return L.clibd_layernorm_fwd(p, 64, 768, p, p, 1e-6, y_bf16, None, None, lora_a, t, 0, 0, 1.0, y_fp8, fp8_scale, None)

    assert ln_fwd(y_fp8=p, fp8_scale=0.0) == -1 and b"positive scale" in L.clibd_last_error()
    assert ln_fwd(y_bf16=p, lora_a=p) == -1 and b"lora_a/t" in L.clibd_last_error()

    def att_fwd(nq=64, out_seq=64, out_fp8_scale=0.0, lse=None, o_lo=None):
        return L.clibd_attention_fwd(p, 2, 64, 2, None, p, nq, out_seq, 0, 0, 1.0, out_fp8_scale, lse, o_lo, None)

    assert att_fwd(lse=p) == -1 and b"together" in L.clibd_last_error()
    assert att_fwd(nq=32, lse=p, o_lo=p) == -1 and b"nq = out_seq = S" in L.clibd_last_error()
    assert att_fwd(out_fp8_scale=2.0, lse=p, o_lo=p) == -1 and b"bf16 out" in L.clibd_last_error()
    assert att_fwd(out_fp8_scale=-1.0) == -1 and b"fp8 scale" in L.clibd_last_error()


def test_reduction_workspace_arguments_are_validated_on_the_host(lib):
    """The workspace rule of the eight reductions that take their partials workspace as an argument (NULL, 0 = the atomic / plain form): a size
    without a workspace, a short and a misaligned workspace are rejected before a launch, and the message names the size query."""
    from clibd_amd import _lib

    L = _lib.load()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(264)   # never dereferenced: every call below is rejected before a launch
    big = 1 << 30
    ep = _lib.GemmEpilogue()
    ep.out_bf16, ep.ld_out_bf16 = 256, 768
    # name -> (call(workspace, workspace_bytes), the size its query asks for); the TN products: the colsum workspace, with colsum_a given
    entries = {
        "gemm_bf16_nt": (lambda ws, n: L.clibd_gemm_bf16_nt(p, 3072, p, 3072, 50432, 768, 3072, ctypes.byref(ep), ws, n, None),
                         L.clibd_gemm_tail_workspace_bytes(50432, 768, 3072)),
        "transpose_colsum_bf16": (lambda ws, n: L.clibd_transpose_colsum_bf16(p, 768, 1000, 768, p, 1024, p, ws, n, None),
                                  L.clibd_transpose_colsum_workspace_bytes(1024, 768)),
        "colsum_bf16": (lambda ws, n: L.clibd_colsum_bf16(p, 768, 1000, 768, p, ws, n, None), L.clibd_colsum_workspace_bytes(1000, 768)),
        "layernorm_param_grads": (lambda ws, n: L.clibd_layernorm_param_grads(p, 0, 768, p, p, 640, 768, p, p, 0, 0, 1.0, ws, n, None),
                                  L.clibd_layernorm_param_grads_workspace_bytes(640, 768)),
        "batch_sum_f32": (lambda ws, n: L.clibd_batch_sum_f32(p, 2048, 768, p, ws, n, None), L.clibd_batch_sum_workspace_bytes(2048, 768)),
        "bert_embed_bwd": (lambda ws, n: L.clibd_bert_embed_bwd(p, None, p, 100, 768, 30522, 2, p, p, ws, n, None),
                           L.clibd_bert_embed_bwd_workspace_bytes(100, 768, 30522, 2)),
        "gemm_bf16_tn_splitk": (lambda ws, n: L.clibd_gemm_bf16_tn_splitk(p, 768, p, 768, 6272, 768, 768, p, 768, 1, p, p, big, ws, n, None),
                                L.clibd_gemm_tn_colsum_workspace_bytes(6272, 768)),
        "gemm_fp8b_tn_splitk": (lambda ws, n: L.clibd_gemm_fp8b_tn_splitk(p, 768, p, 768, 0.5, 6272, 768, 768, p, 768, 1, p, p, big, ws, n, None),
                                L.clibd_gemm_tn_colsum_workspace_bytes(6272, 768)),
    }
    for name, (call, need) in entries.items():
        assert need >= 32, name
        assert call(None, 16) == -1 and b"workspace" in L.clibd_last_error(), name                    # a size without a workspace
        assert call(p, need - 16) == -1, name                                                           # a short workspace
        assert b"too small" in L.clibd_last_error() and b"_workspace_bytes" in L.clibd_last_error(), (name, L.clibd_last_error())
        assert call(odd, big) == -1 and b"misaligned" in L.clibd_last_error(), name                    # 8-byte aligned only
    # the TN products: a colsum workspace goes with colsum_a
    need = L.clibd_gemm_tn_colsum_workspace_bytes(6272, 768)
    assert L.clibd_gemm_bf16_tn_splitk(p, 768, p, 768, 6272, 768, 768, p, 768, 1, None, p, big, p, need, None) == -1
    assert b"colsum_a" in L.clibd_last_error()
    assert L.clibd_gemm_fp8b_tn_splitk(p, 768, p, 768, 0.5, 6272, 768, 768, p, 768, 1, None, p, big, p, need, None) == -1
    assert b"colsum_a" in L.clibd_last_error()
    # three token types: no fixed-order form, so rejected with a workspace; the atomic form takes them (H = 2048 is what stops this call)
    assert L.clibd_bert_embed_bwd(p, p, p, 100, 768, 30522, 3, p, p, p, big, None) == -1 and b"token types" in L.clibd_last_error()
    assert L.clibd_bert_embed_bwd(p, p, p, 100, 2048, 30522, 3, p, p, None, 0, None) == -1
    assert b"token types" not in L.clibd_last_error() and b"H <= 1024" in L.clibd_last_error()


def test_product_path_has_no_cpu_fallback():
    import torch

    from clibd_amd import ops

    with pytest.raises(ValueError):
        ops.l2norm_fwd(torch.zeros(4, 8))
    for py in (ROOT / "clibd_amd").rglob("*.py"):
        assert "oracle" not in re.sub(r"#.*|\"\"\".*?\"\"\"", "", py.read_text(), flags=re.S), f"{py} references the oracle"


def test_gemm256_asynchronous_operands_are_not_touched_before_their_wait():
    """gemm256's epilogue bias is an inline-asm load awaited by an inline-asm s_waitcnt (hipcc does not know the registers are
    written asynchronously): no instruction of any instantiation may touch them in between (tools/check_gemm256_isa.py, hipcc -S)."""
    import importlib.util
    import os

    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed: the ISA cannot be generated here")
    spec = importlib.util.spec_from_file_location("check_gemm256_isa", os.path.join(os.path.dirname(__file__), "..", "tools", "check_gemm256_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main() == 0


def test_hot_kernels_use_no_scratch():
    """Tripwire (round 6): every kernel of the hot units keeps its working set in registers.  A generic-epilogue branch that took a local array by
    pointer once demoted the 256x256 GEMM's 128 accumulators to 528 bytes of scratch per lane — no 'VGPRs Spill' in the compiler's report, no test
    failing, and every generic launch (patch embedding, heads, the whole no-grad forward) 3 x slower.  hipcc cross-compiles without a GPU; the
    units compile in parallel (~75 s).  Allowed: the six attention instantiations whose 2-10 spilled registers were measured faster than their
    spill-free alternatives (profiles/r06_exp_attention_spills.log), none of them on the metric's path."""
    import concurrent.futures as cf

    from clibd_amd import build

    allowed = {   # mangled-name fragment -> scratch bytes per lane it may use
        "attention_fwd_persistent_kernelILi14ELb1ELb1E": 20, "attention_fwd_persistent_kernelILi16ELb1ELb1E": 44, "attention_fwd_persistent_kernelILi16ELb0ELb1E": 12,
        "attention_bwd_kernelILi10ELb0ELb0ELb1ELi4ELi160E": 28, "attention_bwd_kernelILi10ELb0ELb0ELb0ELi4ELi160E": 28, "attention_bwd_kernelILi16ELb1ELb0ELb1ELi4ELi256E": 44,
    }

    units = ["gemm256", "attention", "layernorm", "lora", "gemm", "gemm256_tn", "loss"]
    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        rows = [(k["name"], k["scratch"]) for res in ex.map(build.resource_usage, units) for k in res]
    assert sum(1 for n, _ in rows if "gemm256" in n) >= 40 and len(rows) >= 120, len(rows)
    bad = []
    for name, scratch in rows:
        cap = max([v for k, v in allowed.items() if k in name] or [0])
        if scratch > cap:
            bad.append((name, scratch, cap))
    assert not bad, bad
