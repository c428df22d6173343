"""Compiler-reported resources of pna_batch_plan.hip (hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled here), the way
tests/test_build_resources.py checks the other sources: neither kernel may touch scratch memory (the placement walk unrolls 64 lane
reads and passes its argument block by value: either could end up on the stack without any test noticing), and the workgroup's LDS at the
limits pna_batch_plan_limits reports fits the 160 KiB of a compute unit."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")


def test_no_kernel_of_the_batch_plan_uses_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", str(tmp_path / "out.s"), os.path.join(CSRC, "pna_batch_plan.hip"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", out)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == 2, names
    assert any("k_plan_scan" in n for n in names) and any("k_plan_groups" in n for n in names), names
    assert scratch == [0, 0], list(zip(names, scratch))
    # four wavefronts a workgroup, several workgroups a compute unit at molecule sizes: at most 128 registers keeps four per SIMD
    assert all(v <= 128 for v in vgprs), list(zip(names, vgprs))
    # static LDS (the staged member offsets, one scan row) + the dynamic part at the limits: 4 (2 e + 7 n + 3) bytes
    from pna_amd.graph import batch_plan_limits
    n, e = batch_plan_limits()
    static = lds[[i for i, nm in enumerate(names) if "k_plan_groups" in nm][0]]
    assert static + 4 * (2 * e + 7 * n + 3) <= 160 * 1024
