// The pinhole ray of a pixel, stated once (include/stnerf.h: stnerf_generate_rays_list): generate_rays_list_kernel
// (csrc/accumulate.hip) writes it out, reproject_splat_kernel (csrc/reproject.hip) walks along it.  Every operation is
// generate_rays_kernel's (csrc/sampler.hip), in that kernel's order; contraction is switched off here whatever the file's flags are.
#pragma once
#include "common.h"

namespace stnerf {

#if defined(__HIPCC__)
// kinv = K^-1 (3x3) and T = the pose (4x4), both row-major; pixel p32 of a view w wide, moved by (du, dv).
__device__ __forceinline__ void pinhole_pixel_ray(const float* kinv, const float* T, int p32, int w, float du, float dv, float o[3],
                                                  float d[3]) {
#pragma clang fp contract(off)
    const float u = (float)(p32 % w) + du;  // column
    const float v = (float)(p32 / w) + dv;  // row
    float cx = kinv[0] * u + kinv[1] * v + kinv[2];
    float cy = kinv[3] * u + kinv[4] * v + kinv[5];
    float cz = kinv[6] * u + kinv[7] * v + kinv[8];
    const float nrm = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));  // torch.norm's order (utils/render_helpers.py:108)
    cx = cx / nrm;
    cy = cy / nrm;
    cz = cz / nrm;
    o[0] = T[3];
    o[1] = T[7];
    o[2] = T[11];
    d[0] = T[0] * cx + T[1] * cy + T[2] * cz;
    d[1] = T[4] * cx + T[5] * cy + T[6] * cz;
    d[2] = T[8] * cx + T[9] * cy + T[10] * cz;
}
#endif

}  // namespace stnerf
