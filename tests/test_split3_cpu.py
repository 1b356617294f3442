"""The split-bf16 image and transpose kernels run on every training step.  While they were static copies inside loss.hip,
tests/test_abi.py::test_hot_kernels_use_no_scratch covered them through that unit; they now live in csrc/split3.hip, so the same check is
made here for that unit: the compiler's resource report (no GPU needed) shows both kernels, once each, with no scratch memory."""


def test_split3_kernels_use_no_scratch():
    from clibd_amd import build

    assert "split3" in build.SOURCES
    rows = [(k["name"], k["scratch"]) for k in build.resource_usage("split3")]
    assert sorted(n for n, _ in rows if "split3_image_kernel" in n or "transpose3_bf16_kernel" in n) == sorted(n for n, _ in rows) and len(rows) == 2, rows
    assert all(scratch == 0 for _, scratch in rows), rows
