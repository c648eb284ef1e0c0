// gemmrow_kernel.h instances: IEEE half operands, 16-bit residual streams, K <= 192
#include "gemmrow_kernel.h"
void prx_gemmrow_launch_h6(const prx_gemm_dev::GemmArgs& a, const prx_gemmrow_dev::RowGrid& g, hipStream_t s) {
    prx_gemmrow_dev::launch_slab<half_t, 2, 6>(a, g, s);
}
