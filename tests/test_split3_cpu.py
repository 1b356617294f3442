"""The split-bf16 image and transpose kernels run on every training step.  While they were static copies inside loss.hip,
tests/test_abi.py::test_hot_kernels_use_no_scratch covered them through that unit; they now live in csrc/split3.hip, so the same check is
made here for that unit: the compiler's resource report (no GPU needed) shows both kernels, once each, with no scratch memory."""
import os
import re
import subprocess


def test_split3_kernels_use_no_scratch():
    from clibd_amd import build

    assert "split3" in build.SOURCES
    r = subprocess.run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-Wno-unused-value", "--cuda-device-only", "-c",
                        str(build.CSRC / "split3.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows, name = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|ScratchSize \[bytes/lane\]):\s*(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
        elif name:
            rows.append((name, int(m.group(2))))
    assert sorted(n for n, _ in rows if "split3_image_kernel" in n or "transpose3_bf16_kernel" in n) == sorted(n for n, _ in rows) and len(rows) == 2, rows
    assert all(scratch == 0 for _, scratch in rows), rows
