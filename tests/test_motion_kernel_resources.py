"""Build-quality gate for the split-bf16 MotionNet kernel (mlp_bf16x3_motion_kernel, csrc/mlp_bf16x3.hip), CPU only: hipcc
cross-compiles it to gfx950 assembly.  It runs the stage kernel's MotionNet (motion_bx) over rows of its own, one wave per SIMD;
a value pushed into scratch reloads behind vmcnt(0), i.e. behind the weight ring's DMA queue, inside the K passes."""
import re

import tools.asm_listing as asm


@asm.needs_hipcc
def test_bf16x3_motion_kernel_resources():
    kernels = asm.kernels(asm.listing("mlp_bf16x3.hip"))
    names = [n for n in kernels if re.fullmatch(r"_ZN6stnerf24mlp_bf16x3_motion_kernel\S*", n)]
    assert len(names) == 1, names
    kernel = kernels[names[0]]
    body = kernel["body"]
    assert kernel["ScratchSize"] == 0
    assert kernel["Occupancy"] == 1
    asm.assert_no_scratch_no_call(kernel, names[0])
    # the MotionNet's ring slots as listed: motion_net.0 3, the rolled body of the four 128 x 128 layers 4; 48 MFMAs and 24 operand
    # reads per slot, one barrier and six LDS-DMA per slot (+ the consts' one)
    slots = 3 + 4
    assert body.count("v_mfma_f32_32x32x16_bf16") == 48 * slots, body.count("v_mfma_f32_32x32x16_bf16")
    n_read = len(re.findall(r"ds_read_b128 a\[", body))
    assert 24 * slots <= n_read <= 24 * slots + 6 + 16 * 2, n_read    # + the priming reads, the C-operand (bias) reads
    assert body.count("s_barrier") >= slots and body.count("global_load_lds_dwordx4") >= 6 * slots
