"""The answers of the workspace size queries are part of the C ABI: callers allocate by them, and a fixed-order reduction's partial count
follows from some of them.  The values below were recorded from the library before the workspace layouts moved to the shared Carver
(host_util.h) and the split-bf16 module (split3.hip); a layout change that alters one of them is an ABI change and must say so.
Every set has a shape with all dimensions multiples of 64, one with N / C not multiples of 16, one with a dimension of 1 and the
workload's own shape (2048 x 2048 x 768 for the loss, 916 classes for the head).  Size queries only: no device is needed."""
import ctypes

import pytest

RECORDED = {
    "clibd_softce_workspace_bytes": {(64, 64, 64): 164608, (128, 256, 128): 1115648, (5, 17, 64): 73728, (65, 65, 64): 276480,
                                     (1, 17, 64): 70144, (1, 1, 64): 57856, (2048, 2048, 768): 104882176, (1024, 8192, 768): 219164672},
    "clibd_linear_f32_workspace_bytes": {(64, 64, 64): 166144, (65, 17, 64): 158720, (3, 65, 128): 240640, (1, 1, 64): 57600,
                                         (1, 916, 768): 9368576, (256, 916, 768): 14924288, (2048, 916, 768): 58262016},
    "clibd_ce_rows_workspace_bytes": {(64,): 256, (65,): 512, (1,): 256, (256,): 1024, (2048,): 8192},
    "clibd_ntxent_workspace_bytes": {(128, 64): 101376, (1024, 128): 1712128, (6, 17): 52224, (130, 100): 403456, (4, 1): 52224,
                                     (512, 128): 823296, (4096, 2048): 101220352},
    "clibd_silhouette_workspace_bytes": {(64, 0): 1536, (4096, 64): 4227072, (1000, 128): 136192, (17, 64): 1024, (1, 0): 768, (3, 0): 768,
                                         (20000, 0): 6560256, (20000, 4096): 1760256},
    "clibd_topk_ip_workspace_bytes": {(64, 64): 16, (128, 4096): 262144, (17, 1000): 8704, (1, 1): 16, (1, 100000): 16384,
                                      (1000, 410000): 2048000, (40000, 400000): 16},
    # the last piece is not rounded up and 256 bytes follow it: (17, 1001, 128) and (3, 100000, 768) end on an odd multiple of 128
    "clibd_topk_ip_fast_workspace_bytes": {(64, 64, 64): 16896, (128, 4096, 128): 295680, (17, 1001, 128): 13568, (3, 100000, 768): 54272,
                                           (1, 1, 64): 896, (1, 100000, 64): 17152, (1000, 409600, 768): 9732352},
    "clibd_layernorm_param_grads_workspace_bytes": {(64, 64): 512, (17, 100): 800, (1, 1): 8, (1, 768): 6144, (65, 1024): 16384,
                                                    (403456, 768): 6291456, (272384, 768): 6291456},
    "clibd_layernorm_bwd_pg_workspace_bytes": {(64, 64): 8192, (17, 100): 4000, (1, 1): 8, (1, 768): 6144, (65, 1024): 139264,
                                               (403456, 768): 6291456, (272384, 768): 6291456},
    "clibd_bert_embed_bwd_workspace_bytes": {(64, 64, 1024, 2): 3072, (17, 100, 1000, 2): 4096, (1, 1, 1, 1): 2816, (1, 768, 1027, 2): 14336,
                                             (272384, 768, 1027, 2): 20850688},
}


@pytest.fixture(scope="module")
def lib():
    from clibd_amd import build

    return ctypes.CDLL(str(build.build(verbose=False)))


@pytest.mark.parametrize("query", sorted(RECORDED))
def test_workspace_size_queries_answer_as_recorded(lib, query):
    cases = RECORDED[query]
    assert len(cases) >= 4
    f = getattr(lib, query)
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_int] * len(next(iter(cases)))
    got = {shape: int(f(*shape)) for shape in cases}
    assert got == cases
