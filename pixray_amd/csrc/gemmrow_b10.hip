// gemmrow_kernel.h instances: bf16 operands, fp32 residuals, K <= 320
#include "gemmrow_kernel.h"
void prx_gemmrow_launch_b10(const prx_gemm_dev::GemmArgs& a, const prx_gemmrow_dev::RowGrid& g, hipStream_t s) {
    prx_gemmrow_dev::launch_slab<bf16_t, 1, 10>(a, g, s);
}
