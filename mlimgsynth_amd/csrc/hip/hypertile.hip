// HyperTile: the token rows of a map of H x W tokens brought into tile-major order and back (mlsd_tile_permute, include/mlsd_kernels.h; the plan's users are
// the two permuting copies of mlb_spatial_transf, host/unet.c).  A pure copy of whole rows: no arithmetic, the same kernel for fp16 and fp32 rows.
//   One wave takes one row at a time, in a grid-stride loop over the n_img H W rows.  The row's place on the other side is computed once per row from the wave's
//   row index, which is uniform over the wave (the divisions run on the scalar unit); the lanes then move the row in 16-byte pieces, lane l the pieces l, l + 64, ...:
//   both sides of every wave instruction are one contiguous run of up to 1 KiB.  Rows of the real plans are 1280 .. 5120 bytes (80 .. 320 pieces); up to four pieces
//   per lane are loaded before the first is stored, so that a wave keeps a whole 4 KiB of a row in flight.
//   All offsets are 64-bit: 8 x 16384 rows of 5120 bytes do not fit 2^31.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

constexpr int kWaves = 4;       // waves per block

// tile-major row index of the image-order row (img, py, px): ((img nh + ty) nw + tx) th tw + y tw + x
struct TileGeom { int H, W, th, tw, nw; long hw; };

__device__ __forceinline__ long tiled_of_image_row(long r, const TileGeom& g)
{
    const long img = r / g.hw;
    const int q = (int)(r - img * g.hw);
    const int py = q / g.W, px = q - py * g.W;
    const int ty = py / g.th, y = py - ty * g.th;
    const int tx = px / g.tw, x = px - tx * g.tw;
    return img * g.hw + ((long)(ty * g.nw + tx) * g.th + y) * g.tw + x;
}

// rows are indexed in IMAGE order; INVERSE only swaps which side is read
template <bool INVERSE>
__global__ __launch_bounds__(64 * kWaves) void tile_permute_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, long n_rows, TileGeom g, int pieces)
{
    const int lane = (int)(threadIdx.x & 63);
    const long wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long)blockIdx.x * kWaves;
    const long n_waves = (long)gridDim.x * kWaves;
    for (long r = wave0; r < n_rows; r += n_waves) {
        const long t = tiled_of_image_row(r, g);
        const u32x4* __restrict__ s = src + (INVERSE ? t : r) * pieces;
        u32x4* __restrict__ d = dst + (INVERSE ? r : t) * pieces;
        int p = lane;
        for (; p + 192 < pieces; p += 256) {
            const u32x4 a = s[p], b = s[p + 64], c = s[p + 128], e = s[p + 192];
            d[p] = a; d[p + 64] = b; d[p + 128] = c; d[p + 192] = e;
        }
        for (; p < pieces; p += 64) d[p] = s[p];
    }
}

}  // namespace

extern "C" MLSD_API int mlsd_tile_permute(const void* src, void* dst, int n_img, int H, int W, int th, int tw, int row_bytes, int inverse, void* stream)
{
    if (!src || !dst || n_img < 1 || H < 1 || W < 1 || th < 1 || tw < 1 || row_bytes < 16)
        return mlsd_set_error(-1, "mlsd_tile_permute: bad argument (%d maps of %d x %d rows of %d bytes, tiles of %d x %d)", n_img, H, W, row_bytes, th, tw);
    if (H % th || W % tw) return mlsd_set_error(-1, "mlsd_tile_permute: tiles of %d x %d do not divide a map of %d x %d", th, tw, H, W);
    if (row_bytes % 16) return mlsd_set_error(-1, "mlsd_tile_permute: rows of %d bytes (a multiple of 16)", row_bytes);
    if (((uintptr_t)src | (uintptr_t)dst) & 15) return mlsd_set_error(-1, "mlsd_tile_permute: pointers must be 16-byte aligned");
    if ((long)H * W >= (1L << 31)) return mlsd_set_error(-1, "mlsd_tile_permute: more than 2^31 rows per map");
    const long n_rows = (long)n_img * H * W;
    const size_t total = (size_t)n_rows * (size_t)row_bytes;
    const char *s0 = (const char*)src, *d0 = (const char*)dst;
    if (s0 < d0 + total && d0 < s0 + total) return mlsd_set_error(-1, "mlsd_tile_permute: source and destination overlap");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("tile_permute");      // the dry runtime's buffers are host memory: refuse before the launch
    TileGeom g; g.H = H; g.W = W; g.th = th; g.tw = tw; g.nw = W / tw; g.hw = (long)H * W;
    long blocks = (n_rows + kWaves - 1) / kWaves;
    if (blocks > 4096) blocks = 4096;      // 16 waves per CU on 256 CUs; the rest of the rows in the grid-stride loop
    const dim3 grid((unsigned)blocks), block(64 * kWaves);
    if (inverse) hipLaunchKernelGGL(tile_permute_kernel<true>, grid, block, 0, (hipStream_t)stream, (const u32x4*)src, (u32x4*)dst, n_rows, g, row_bytes / 16);
    else hipLaunchKernelGGL(tile_permute_kernel<false>, grid, block, 0, (hipStream_t)stream, (const u32x4*)src, (u32x4*)dst, n_rows, g, row_bytes / 16);
    return mlsd_check_launch("tile_permute");
}
