// The row-list flavour of the split-bf16 stage kernel (mlp_bf16x3_stage_kernel.h under a name of its own): a queue slot with a row
// list walks *row_count packed words (ray << 8 | k) instead of hit rays x samples (the sample cull).  A file
// of its own, so that mlp_bf16x3.hip holds the kernels it always held.
#define STNERF_STAGE_KERNEL mlp_bf16x3_stage_rows_kernel
#include "mlp_bf16x3_stage_kernel.h"

namespace stnerf {

int launch_bf16x3_stage_rows(const StageArgs& a, const StageRowsArgs& r, bool deep_rgb, int cus, hipStream_t stream) {
    const int64_t max_items = ((a.n_rays * a.ns + WV_ITEM - 1) / WV_ITEM) * a.n_layers;
    const int grid = (int)(max_items < cus ? max_items : cus);  // one persistent workgroup per CU
    const void* kfn = deep_rgb ? reinterpret_cast<const void*>(mlp_bf16x3_stage_rows_kernel<true, StageRowsArgs>)
                               : reinterpret_cast<const void*>(mlp_bf16x3_stage_rows_kernel<false, StageRowsArgs>);
    if (const int rc = reserve_dynamic_lds(kfn, BX_LDS, "mlp_stage_rows (bf16x3)")) return rc;
    if (deep_rgb)
        hipLaunchKernelGGL((mlp_bf16x3_stage_rows_kernel<true, StageRowsArgs>), dim3(grid), dim3(WV_THREADS), BX_LDS, stream, a, r);
    else
        hipLaunchKernelGGL((mlp_bf16x3_stage_rows_kernel<false, StageRowsArgs>), dim3(grid), dim3(WV_THREADS), BX_LDS, stream, a, r);
    STNERF_CHECK_LAUNCH("mlp_stage_rows (bf16x3)");
    return STNERF_OK;
}

}  // namespace stnerf
