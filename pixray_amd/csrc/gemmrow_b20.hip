// gemmrow_kernel.h instances: bf16 operands, fp32 residuals, 320 < K <= 640, 80-column slabs
#include "gemmrow_kernel.h"
void prx_gemmrow_launch_b20(const prx_gemm_dev::GemmArgs& a, const prx_gemmrow_dev::RowGrid& g, hipStream_t s) {
    prx_gemmrow_dev::launch_slab<bf16_t, 1, 20>(a, g, s);
}
