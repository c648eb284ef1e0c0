// gemmrowconv_kernel.h instances: bf16 operands
#include "gemmrowconv_kernel.h"
void prx_gemmrowconv_launch_b(const prx_gemm_dev::GemmArgs& a, int shape, int row_tiles, int n_cu, hipStream_t s) {
    prx_gemmrow_dev::launch_conv<bf16_t>(a, shape, row_tiles, n_cu, s);
}
