// Host side of the row-streaming GEMM kernels (gemmrow_kernel.h, gemmrowconv_kernel.h): which kernel takes a descriptor, launch geometry,
// dispatch to the instance units.  The kernels that exist are stated once, in those headers (row_slab_tiles, row_k_bucket,
// row_kernel_exists; kRowConvShapes, row_conv_act); the plan here accepts by them and the launch instantiates by them.
#include "gemmrowconv_kernel.h"
#include <algorithm>
#include <atomic>
#include <cassert>
#include <cstdlib>

using namespace prx_gemmrow_dev;

namespace {
std::atomic<long long> g_row_launches{0};
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

// (Whether a problem is LARGE enough is the caller's rule: GemmCtx::rowk_min.)
bool prx_gemmrow_plan(const GemmDesc& d, int* nt, int* ksm) {
    if (d.f32 || d.a_is_f32 || d.bias_m || d.gn_stats || d.gnb_x || d.out_bf16_pre) return false;
    if (!al16(d.A) || !al16(d.B) || d.lda % 8 != 0 || d.ldb % 8 != 0) return false;
    if (d.out_f32 && (!al16(d.out_f32) || d.ldc_f32 % 4 != 0)) return false;
    if (d.out_bf16 && (!al16(d.out_bf16) || d.ldc_bf16 % 8 != 0)) return false;
    if (!d.out_f32 && !d.out_bf16) return false;
    const bool has_aux = d.act == PRX_ACT_MUL_RELUMASK || d.act == PRX_ACT_RELUMASK_POST;
    if (has_aux && (!d.aux || !al16(d.aux) || d.ldaux % 8 != 0)) return false;
    if (d.a_mode == PRX_A_CONV3X3) {
        // implicit 3x3 convolutions of the listed shapes, no residual
        const int shape = row_conv_shape(d.N, d.Cin);
        if (d.up != 0 || shape < 0 || d.K != 9 * d.Cin || d.resid || !row_conv_act(d.act)) return false;
        if ((size_t)d.M * d.lda * 2 >= ((size_t)1 << 31)) return false;          // 32-bit tap offsets inside one image are always fine; keep the map addressable
        *nt = kRowConvShapes[shape].nt; *ksm = 0;
        return true;
    }
    if (d.a_mode != PRX_A_ROWMAJOR || d.K % 8 != 0) return false;
    const int ksteps = (d.K + 31) / 32, slab = row_slab_tiles(d.N, ksteps), bucket = row_k_bucket(ksteps);
    if (slab == 0 || bucket == 0 || !row_kernel_exists(d.act, d.resid != nullptr, slab, bucket)) return false;
    if (d.resid && ((d.row16 & 1) != 0) != (d.h16 != 0)) return false;       // half: 16-bit residual streams; bf16: fp32 residuals
    if (d.resid && (!al16(d.resid) || d.ldr % 8 != 0)) return false;
    *nt = slab; *ksm = bucket;
    return true;
}

void prx_gemmrow_launch(const prx_gemm_dev::GemmArgs& a, int nt, int ksm, int n_cu, hipStream_t s) {
    const GemmDesc& d = a.d;
    const int row_tiles = (d.M + 15) / 16, cus = n_cu > 0 ? n_cu : 256;
    if (d.a_mode == PRX_A_CONV3X3) {
        // one persistent workgroup per CU, each on a contiguous run of 16-pixel tiles (neighbouring image rows: the 9 taps of a pixel
        // are fetched from HBM once and from the L2 of the chunk's XCD after that... as far as the round-robin of workgroups allows)
        const int shape = row_conv_shape(d.N, d.Cin);
        assert(shape >= 0 && row_conv_act(d.act));        // prx_gemmrow_plan accepted d by the same table
        (d.h16 ? prx_gemmrowconv_launch_h : prx_gemmrowconv_launch_b)(a, shape, row_tiles, cus, s);
        g_row_launches.fetch_add(1, std::memory_order_relaxed);
        return;
    }
    assert(row_kernel_exists(d.act, d.resid != nullptr, nt, ksm));     // prx_gemmrow_plan accepted d by the same predicate
    RowGrid g;
    g.nt = nt; g.ksteps = (d.K + 31) / 32; g.nslab = d.N / (nt * 16); g.row_tiles = row_tiles;
    // one workgroup of 8 waves per CU (the kernels hold 130 - 220 registers: two waves per SIMD); the grid is a whole number of
    // (8 XCDs x nslab) groups
    static const int per_cu = [] { const char* e = getenv("PRX_GEMM_ROWK_WGS"); return e ? std::max(1, atoi(e)) : 1; }();
    const int group = 8 * g.nslab;
    // (the 80-column slabs: <= 128 registers and 32 / 52 KB of LDS -- two workgroups per CU keep more of their long activation rows in flight)
    const int wgs = (nt == 5 && ksm <= 10) ? 2 * per_cu : per_cu;
    g.grid = std::max(1, (wgs * cus) / group) * group;
    g.nchunks = (g.grid / group) * 8;
    static void (*const launch[2][3])(const prx_gemm_dev::GemmArgs&, const RowGrid&, hipStream_t) = {
        {prx_gemmrow_launch_b6, prx_gemmrow_launch_b10, prx_gemmrow_launch_b20}, {prx_gemmrow_launch_h6, prx_gemmrow_launch_h10, prx_gemmrow_launch_h20}};
    launch[d.h16 ? 1 : 0][ksm == 6 ? 0 : (ksm == 10 ? 1 : 2)](a, g, s);
    g_row_launches.fetch_add(1, std::memory_order_relaxed);
}

long long prx_gemmrow_launches() { return g_row_launches.load(std::memory_order_relaxed); }
extern "C" long long prx_gemm_row_launches(void) { return prx_gemmrow_launches(); }
