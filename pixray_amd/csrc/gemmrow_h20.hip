// gemmrow_kernel.h instances: IEEE half operands, 16-bit residual streams, 320 < K <= 640, 80-column slabs
#include "gemmrow_kernel.h"
void prx_gemmrow_launch_h20(const prx_gemm_dev::GemmArgs& a, const prx_gemmrow_dev::RowGrid& g, hipStream_t s) {
    prx_gemmrow_dev::launch_slab<half_t, 2, 20>(a, g, s);
}
