"""Build-quality gate for the lookup kernel of the grid proposals (csrc/proposal.hip), CPU only, in the manner of
tests/test_deep_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and the code
object's own metadata is read -- register counts, scratch and LDS, nothing else.

proposal_density_kernel gathers eight vertices per sample and is bound by those loads: it wants every wave slot, so at most 128
VGPRs (four waves per SIMD), no scratch, no spills and no LDS.  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): 70 VGPRs
(the sample loop is unrolled twice), occupancy 7."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _kernels(text):
    """{symbol: (VGPRs, scratch bytes, occupancy, LDS bytes, spilled VGPRs, spilled SGPRs)} of every kernel of an assembly listing."""
    out = {}
    for name in re.findall(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(name + ":"):]
        if "s_endpgm" not in tail:
            continue
        body = tail[:tail.index("s_endpgm")]
        get = lambda k: int(re.search(r"; " + k + r": (\d+)", tail).group(1))
        assert "scratch_" not in body and "s_swappc" not in body, name
        meta = text[text.index(".name:", text.index("amdhsa.kernels")):]      # (one kernel in the file: its metadata record)
        spill = lambda k: int(re.search(r"\." + k + r"_spill_count:\s*(\d+)", meta).group(1))
        out[name] = (get("TotalNumVgprs"), get("ScratchSize"), get("Occupancy"), get("LDSByteSize"), spill("vgpr"), spill("sgpr"))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")
def test_the_lookup_kernel_uses_no_scratch_no_spills_no_lds_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "proposal.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "proposal.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    text = open(asm).read()
    kernels = _kernels(text)
    assert len(kernels) == 1 and "proposal_density_kernel" in next(iter(kernels)), sorted(kernels)
    for name, (vgprs, scratch, occupancy, lds, vspill, sspill) in kernels.items():
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}, spills {vspill} / {sspill}")
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert lds == 0, (name, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
    body = text[text.index(next(iter(kernels)) + ":"):]
    body = body[:body.index("s_endpgm")]
    assert "v_fma_f32" not in body and "v_fmac_f32" not in body and "v_pk_fma_f32" not in body      # every product and sum on its own
    assert "global_store_dwordx4" in body                                                          # one float4 store per sample
    from stnerf_amd import build
    assert ("proposal.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
