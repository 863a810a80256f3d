"""Build-quality gate for the kernel of the lens model in ray generation (csrc/lens.hip), CPU only, in the manner of
tests/test_accumulate_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and
the code object's own metadata is read.

One helper kernel, generate_rays_lens_kernel (one lane per row, HBM-bound on the row it writes).  It must use no scratch, at most
128 VGPRs with an occupancy of at least 4 -- the bar of the other helper kernels -- and no LDS.  Measured with hipcc
--offload-arch=gfx950 (ROCm 7.2): the figures are printed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("generate_rays_lens_kernel",)


def _kernels(text):
    """{symbol: (VGPRs, scratch bytes, occupancy, LDS bytes)} of every kernel of an assembly listing."""
    out = {}
    for name in re.findall(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(name + ":"):]
        if "s_endpgm" not in tail:
            continue
        body = tail[:tail.index("s_endpgm")]
        get = lambda k: int(re.search(r"; " + k + r": (\d+)", tail).group(1))
        assert "scratch_" not in body and "s_swappc" not in body, name
        out[name] = (get("TotalNumVgprs"), get("ScratchSize"), get("Occupancy"), get("LDSByteSize"))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")
def test_the_lens_kernel_uses_no_scratch_no_lds_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "lens.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "lens.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    text = open(asm).read()
    kernels = _kernels(text)
    assert len(kernels) == len(KERNELS) and all(sum(k in name for name in kernels) == 1 for k in KERNELS), sorted(kernels)
    for name, (vgprs, scratch, occupancy, lds) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        assert lds == 0, (name, lds)
    # the definition's products, quotients and sums stay separate fp32 operations: the file is built without contraction.  A
    # correctly rounded fp32 quotient and square root are themselves EXPANDED into fused operations, so a probe kernel of one
    # quotient and one of one root are compiled with the same flags, and the kernel must hold exactly the fused operations of its
    # quotients and roots plus the two fmaf it WRITES (the squared norm in torch.norm's order) -- one more would be a contracted
    # product of ours.  Quotients in the listing: xd, yd, the round's two (the loop is not unrolled), focus / cz, the norm's three.
    probe = tmp_path / "probe.hip"
    probe.write_text("#include <hip/hip_runtime.h>\n"
                     "__global__ void probe_div(const float* a, const float* b, float* o) { o[threadIdx.x] = a[threadIdx.x] / b[threadIdx.x]; }\n"
                     "__global__ void probe_sqrt(const float* a, float* o) { o[threadIdx.x] = sqrtf(a[threadIdx.x]); }\n")
    probe_asm = str(tmp_path / "probe.s")
    assert subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", probe_asm,
                           str(probe)], stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    probe_text = open(probe_asm).read()

    def fused(listing, name):
        body = listing[listing.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        return (len(re.findall(r"\bv_(?:pk_)?(?:fma|mac|fmac)\w*_f32", body)), len(re.findall(r"\bv_div_fixup_f32", body)),
                len(re.findall(r"\bv_sqrt_f32", body)))
    per_div, one, _ = fused(probe_text, [n for n in re.findall(r"^(_Z\w+):", probe_text, re.M) if "probe_div" in n][0])
    per_sqrt, _, one_root = fused(probe_text, [n for n in re.findall(r"^(_Z\w+):", probe_text, re.M) if "probe_sqrt" in n][0])
    assert one == 1 and one_root == 1
    for name in sorted(kernels):
        n_fused, n_div, n_sqrt = fused(text, name)
        print(f"{name}: {n_fused} fused operations, {n_div} quotients, {n_sqrt} roots")
        assert (n_div, n_sqrt) == (8, 1), (name, n_div, n_sqrt)
        assert n_fused == per_div * n_div + per_sqrt * n_sqrt + 2, (name, n_fused, per_div, per_sqrt)
    from stnerf_amd import build
    assert ("lens.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
