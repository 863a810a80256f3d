"""Build-quality gate for the split-bf16 MotionNet kernel (mlp_bf16x3_motion_kernel, csrc/mlp_bf16x3.hip), CPU only: hipcc
cross-compiles it to gfx950 assembly.  It runs the stage kernel's MotionNet (motion_bx) over rows of its own, one wave per SIMD;
a value pushed into scratch reloads behind vmcnt(0), i.e. behind the weight ring's DMA queue, inside the K passes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")
def test_bf16x3_motion_kernel_resources(tmp_path):
    src = os.path.join(ROOT, "st-nerf_amd", "csrc", "mlp_bf16x3.hip")
    asm = tmp_path / "mlp_bf16x3.s"
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "-S", "--cuda-device-only", "-o", str(asm), src]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = asm.read_text()
    names = re.findall(r"^(_ZN6stnerf24mlp_bf16x3_motion_kernel\S*):", text, re.M)
    assert len(names) == 1, names
    tail = text[text.index(names[0] + ":"):]
    body = tail[:tail.index("s_endpgm")]
    assert int(re.search(r"; ScratchSize: (\d+)", tail).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", tail).group(1)) == 1
    assert "scratch_" not in body and "s_swappc" not in body
    # the MotionNet's ring slots as listed: motion_net.0 3, the rolled body of the four 128 x 128 layers 4; 48 MFMAs and 24 operand
    # reads per slot, one barrier and six LDS-DMA per slot (+ the consts' one)
    slots = 3 + 4
    assert body.count("v_mfma_f32_32x32x16_bf16") == 48 * slots, body.count("v_mfma_f32_32x32x16_bf16")
    n_read = len(re.findall(r"ds_read_b128 a\[", body))
    assert 24 * slots <= n_read <= 24 * slots + 6 + 16 * 2, n_read    # + the priming reads, the C-operand (bias) reads
    assert body.count("s_barrier") >= slots and body.count("global_load_lds_dwordx4") >= 6 * slots
