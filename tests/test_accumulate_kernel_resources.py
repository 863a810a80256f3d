"""Build-quality gate for the kernels of progressive multi-sample frames (csrc/accumulate.hip), CPU only, in the manner of
tests/test_occluder_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and
the code objects' own metadata is read.

Six helper kernels, all HBM-bound or tiny: generate_rays_list_kernel (one lane per row), accumulate_kernel (one lane per (row,
column): consecutive lanes touch consecutive floats) and accumulate_count_kernel, and the three launches of the ordered
compaction, select_count_kernel / select_scan_kernel / select_write_kernel.  Every one must use no scratch and at most 128 VGPRs
with an occupancy of at least 4 -- the bar of the other helper kernels; the accumulator and the ray generator use no LDS, the
three select kernels a few words of it (the waves' popcounts; the scan's 16 wave sums and its carry).  Measured with hipcc
--offload-arch=gfx950 (ROCm 7.2): the figures are printed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("generate_rays_list_kernel", "accumulate_kernel", "accumulate_count_kernel", "select_count_kernel", "select_scan_kernel",
           "select_write_kernel")


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
def test_the_accumulate_kernels_use_no_scratch_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "accumulate.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "accumulate.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    text = open(asm).read()
    kernels = _kernels(text)
    assert len(kernels) == len(KERNELS) and all(sum(k in name for name in kernels) == 1 for k in KERNELS), sorted(kernels)
    for name, (vgprs, scratch, occupancy, lds) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        if "select_" in name:
            assert lds <= 128, (name, lds)
        else:
            assert lds == 0, (name, lds)
    # the definitions' products, quotients and sums stay separate fp32 operations: the file is built without contraction.  That
    # test's check (no fused multiply-add at all) needs one allowance here: a correctly rounded fp32 quotient and square root are
    # themselves EXPANDED into fused operations (the ray generator divides three times and takes one root, the accumulator
    # divides once).  So a probe kernel of one quotient and one of one root are compiled with the same flags, and every kernel
    # must hold exactly the fused operations of its quotients and roots -- one more would be a contracted product of ours.  The ray
    # generator adds the two fmaf it WRITES: the squared norm in torch.norm's order, fmaf(z, z, fmaf(y, y, x x))
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
    expected = {"generate_rays_list_kernel": (3, 1), "accumulate_kernel": (1, 0)}
    for name in sorted(kernels):
        n_fused, n_div, n_sqrt = fused(text, name)
        want = next((v for k, v in expected.items() if k in name), (0, 0))
        print(f"{name}: {n_fused} fused operations, {n_div} quotients, {n_sqrt} roots")
        assert (n_div, n_sqrt) == want, (name, n_div, n_sqrt)
        written = 2 if "generate_rays_list_kernel" in name else 0
        assert n_fused == per_div * n_div + per_sqrt * n_sqrt + written, (name, n_fused, per_div, per_sqrt, written)
    from stnerf_amd import build
    assert ("accumulate.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
