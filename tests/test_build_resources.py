"""Compiler-reported resources of the hot kernels (hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled here): no
kernel may touch scratch memory.  A lambda that silently stops being inlined makes the by-value argument block (or the
accumulators, through a run-time panel index) live on the stack -- the contraction of the tower layers ran 8x slower that
way for a while without any test noticing."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")


# The bf16 gather (pna_bf16_gather.hip), per instantiation <V8, VOUT, MSG> / <V8, MSG>: the plain gather of big graphs (MSG = false)
# keeps >= 5 wavefronts per SIMD (<= 96 registers) and must not inherit the message fold's ~144; the message gather stays on its
# step of 3 wavefronts per SIMD (<= 168).
_B = ("Lb0E", "Lb1E")
BF16_GATHER_CAPS = {f"k_gather_bf16{kern}Lb{msg}EEE": cap for msg, cap in ((0, 96), (1, 168))
                    for kern in [f"I{v}{o}" for v in _B for o in _B] + [f"_segI{v}" for v in _B]}


# (the grouped one-block kernel runs two 8-wavefront workgroups per CU: above 128 registers it would silently drop to one; the
#  three-block grouped kernel runs 12 wavefronts per CU: 168)
@pytest.mark.parametrize("src,max_vgpr", [("pna_posttrans_x3.hip", {"k_posttrans_x3": 256, "k_posttrans_x3ILi1ELb0ELi80ELi5ELi1ELi8ELi3ELb0ELb1EEE": 128,
                                                                    "k_posttrans_x3ILi3ELb0ELi80ELi5ELi1ELi12ELi3ELb0ELb1EEE": 168}), ("pna_segreduce.hip", {"k_segreduce_fastILi4ELb0ELb0ELb0ELi0ELb0E": 80, "k_segreduce_fastILi4ELb1ELb0ELb0ELi0ELb0E": 80, "k_segreduce_fastILi4ELb1ELb1ELb0ELi0ELb0E": 80,
                                                                                        # (the 64-bit-address instantiations for source tables beyond 2^24 rows / 4 GiB: five wavefronts per SIMD)
                                                                                        "k_segreduce_fastILi4ELb0ELb0ELb0ELi0ELb1E": 80, "k_segreduce_fastILi4ELb1ELb0ELb0ELi0ELb1E": 88, "k_segreduce_fastILi4ELb1ELb1ELb0ELi0ELb1E": 88,
                                                                                        # (the arg-tracking instantiations of the training forward and the edge-term ones: four to five wavefronts per SIMD)
                                                                                        "k_segreduce_fastILi4ELb0ELb0ELb1ELi0E": 104, "k_segreduce_fastILi4ELb1ELb0ELb1ELi0E": 104,
                                                                                        "k_segreduce_fastILi4ELb1ELb0ELb0ELi1E": 104, "k_segreduce_fastILi4ELb1ELb0ELb0ELi2E": 104}),
                                          ("pna_posttrans.hip", {}), ("pna_pack.hip", {}), ("pna_tower_fused.hip", {}), ("pna_fused.hip", {}),
                                          ("pna_segreduce_bwd.hip", {}),
                                          # the resident-weight projections: one 8-wavefront workgroup per CU (126 KB of LDS), 256 registers each
                                          ("pna_project.hip", {"k_project": 256}),
                                          # the weight-gradient kernels: two 4-wavefront workgroups / one 8-wavefront workgroup per CU
                                          ("pna_posttrans_dw.hip", {"k_posttrans_dw": 256}),
                                          # the one-kernel layer: two 4-wavefront workgroups per CU (the production instantiations: DUMP = false)
                                          # (incl. the tower instantiations ...ELb0ELb1ELb0EEE of the two-full-block shapes)
                                          ("pna_fused_degree.hip", {"k_fused_degreeILi1ELb0ELb0E": 256, "k_fused_degreeILi1ELb1ELb0E": 256,
                                                                    "k_fused_degreeILi2ELb0ELb0E": 256, "k_fused_degreeILi2ELb1ELb0E": 256}),
                                          # the bf16 inference family (new entries go LAST: the test ids carry the position); the
                                          # contraction has no cap (its accumulators sit in AGPRs), the one-call layer stays at 3
                                          # wavefronts per SIMD
                                          ("pna_bf16_gather.hip", BF16_GATHER_CAPS), ("pna_bf16_contract.hip", {}),
                                          ("pna_bf16_small.hip", {"k_tower_rows_bf16": 168})])
def test_no_kernel_uses_scratch(src, max_vgpr, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", str(tmp_path / "out.s"), os.path.join(CSRC, src), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", out)]
    assert names and len(names) == len(scratch) == len(vgprs)
    # k_heavy_finalize (a 25 us kernel over the ~3 k hub rows) indexes its per-aggregator result arrays with the run-time
    # aggregator code and keeps them in scratch: known, not on the hot path
    # the generic-epilogue instantiation of the 128-column contraction (the second launch over the <= 15 tail rows of M % 16)
    # keeps 28 B of its epilogue state in scratch at the 256-register ceiling: <= 32 B tolerated there and only there
    tail_128 = re.compile(r"k_posttrans_x3ILi\dELb[01]ELi128E.*ELb1ELb0EEE")
    bad = [(n, s) for n, s in zip(names, scratch)
           if s != 0 and "k_heavy_finalize" not in n and not (tail_128.search(n) and s <= 32)]
    assert not bad, f"kernels using scratch: {bad[:5]}"
    for key, lim in max_vgpr.items():
        assert any(key in n for n in names), f"no kernel named {key}"
        over = [(n, v) for n, v in zip(names, vgprs) if key in n and v > lim]
        assert not over, over[:5]
    # every inline-asm memory instruction of every kernel: no SGPR operand written by a VALU instruction (an SGPR-spill reload)
    # fewer than five wait states before it (tools/isa_audit.py::sgpr_hazards; hipcc does not check inside inline asm)
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    text = open(str(tmp_path / "out.s")).read()
    for n in names:
        kl = isa_audit.kernel_lines(str(tmp_path / "out.s"), n)
        haz = isa_audit.sgpr_hazards(kl)
        assert not haz, (n, haz[:5])
        # ... and, in a source whose kernels issue MFMAs (wavefronts of ONE launch share SIMDs): no packed-fp32 instruction whose low
        # lane reads src1's high half -- on gfx950 it drops its low-half result in lanes 48-63 beside an MFMA wavefront
        # (tools/ubench/pk_opsel_mfma_repro.hip); hipcc emits the form on its own when it vectorises scalar code
        if "v_mfma" in text:
            pk = isa_audit.pk_src1_hi_selects(kl)
            assert not pk, (n, pk[:5])


def test_one_kernel_layer_never_touches_a_register_in_flight(tmp_path):
    """pna_fused_degree.hip issues every gather load through inline asm and waits for it with counted s_waitcnt: hipcc neither
    counts those loads nor knows that their destination registers are not valid yet.  tools/isa_audit.py replays the compiled
    kernel's control-flow graph and reports any instruction -- compiler-generated or ours -- that reads or writes a register whose
    load (VMEM, LDS or scalar) is still in flight.  All instantiations, production and verification."""
    import sys
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    out = str(tmp_path / "fd.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "pna_fused_degree.hip")], check=True, capture_output=True)
    names = sorted(set(re.findall(r"^(_ZN\S*k_fused_degreeI\S+?):", open(out).read(), flags=re.M)))
    # (4 shapes + 3 wide ones) x (fp16 x 2 production, fp16 x 2 verification, bf16 x 3 production) + 2 tower shapes x (fp16 x 2, bf16 x 3)
    assert len(names) == 25, names
    for n in names:
        kl = isa_audit.kernel_lines(out, n)
        probs = isa_audit.audit(kl)
        assert not probs, (n, probs[:5])
        # ... nor hands an inline-asm memory instruction an SGPR (a base pointer) that a VALU instruction -- the v_readlane_b32 of
        # an SGPR-spill reload -- wrote fewer than five wait states before: hipcc's hazard recognizer does not look inside inline asm
        haz = isa_audit.sgpr_hazards(kl)
        assert not haz, (n, haz[:5])


def test_resident_weight_projection_never_touches_a_register_in_flight(tmp_path):
    """pna_project.hip requests the next tile's row windows through inline asm one tile ahead and waits with its own s_waitcnt: the same
    replay (tools/isa_audit.py) over every instantiation of both kernels."""
    import sys
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    out = str(tmp_path / "pj.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "pna_project.hip")], check=True, capture_output=True)
    names = sorted(set(re.findall(r"^(_ZN\S*k_project\S+?):", open(out).read(), flags=re.M)))
    assert len(names) == 8 + 8 * 3 + 5 + 8, names                # K chunks 1..8 x (plain, 1..3 blocks, grouped) + four blocks at <= 5 chunks
    for n in names:
        kl = isa_audit.kernel_lines(out, n)
        probs = isa_audit.audit(kl)
        assert not probs, (n, probs[:5])
        haz = isa_audit.sgpr_hazards(kl)
        assert not haz, (n, haz[:5])
