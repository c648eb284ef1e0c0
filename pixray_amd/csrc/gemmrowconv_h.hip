// gemmrowconv_kernel.h instances: IEEE half operands
#include "gemmrowconv_kernel.h"
void prx_gemmrowconv_launch_h(const prx_gemm_dev::GemmArgs& a, int shape, int row_tiles, int n_cu, hipStream_t s) {
    prx_gemmrow_dev::launch_conv<half_t>(a, shape, row_tiles, n_cu, s);
}
