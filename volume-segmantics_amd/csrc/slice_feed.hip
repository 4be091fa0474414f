// Training feed straight from resident volumes (gfx950; HBM-bound byte work): the fitted (size x size) uint8 slice pairs that
// data/datasets.py:fit_to_square makes of the PNG slices, cut out of the uint8 data / label volumes where they lie in HBM.  One
// launch serves a batch that mixes volumes, axes and slice indices: every sample brings its own descriptor (vs_slice_cut), whose
// fitted size, pad offsets and border mode the HOST computed with fit_to_square's own expressions - nothing is re-derived here.
// Per output pixel:
//   pad     the centred np.pad: reflect-101, periodic when the pad is wider than the slice ("reflect"), or the clamped index ("edge")
//   scale   LongestMaxSize: the image through cv2.resize's bilinear form (resample.h, the sampler of the augmentations), the
//           mask through its nearest form floor(dst * scale); a slice that already has the fitted size is copied
// data/volume_feed.py:cut_numpy is the NumPy form of the same arithmetic (CPU devices + tests).
// A thread makes four neighbouring pixels of a row and stores them as one 32-bit word per output; reads are byte gathers (slices
// along x touch one byte per line).  Measured for 32 slices of 256^2 (profiles/volume_feed.txt): 17 us per batch along z and y,
// 20 us along x, against a training step of 5.7 ms in the same run.
#include "common.h"
#include "resample.h"

namespace {

__device__ __forceinline__ int pad_index(int i, int n, int border) { return border ? min(max(i, 0), n - 1) : refl101(i, n); }

// whether every address the descriptor can produce lies inside a buffer of `elems` elements
__device__ __forceinline__ bool cut_in_bounds(int64_t off, const vs_slice_cut& d, int64_t elems) {
    if (off < 0 || d.row_stride < 0 || d.col_stride < 0) return false;
    // in fp64: exact below 2^53, and a product that would wrap an int64 is far above any buffer size
    return (double)off + (double)(d.h - 1) * (double)d.row_stride + (double)(d.w - 1) * (double)d.col_stride < (double)elems;
}

__global__ __launch_bounds__(256) void slices_cut_kernel(const uint8_t* __restrict__ data, const uint8_t* __restrict__ labels,
                                                        int64_t data_elems, int64_t label_elems,
                                                        const vs_slice_cut* __restrict__ table, int size,
                                                        uint8_t* __restrict__ images, uint8_t* __restrict__ masks) {
    const int b = blockIdx.y;
    const vs_slice_cut d = table[b];
    const int qw = size >> 2, quads = size * qw;
    uint32_t* oi = reinterpret_cast<uint32_t*>(images + (size_t)b * size * size);
    uint32_t* om = reinterpret_cast<uint32_t*>(masks + (size_t)b * size * size);
    // (the loader validates its table on the host and raises; a descriptor that would still read outside the volumes reads nothing)
    const bool ok = d.h >= 1 && d.w >= 1 && d.nh >= 1 && d.nw >= 1 && cut_in_bounds(d.img_off, d, data_elems) &&
                    cut_in_bounds(d.msk_off, d, label_elems);
    const uint8_t* si = data + (ok ? d.img_off : 0);
    const uint8_t* sm = labels + (ok ? d.msk_off : 0);
    const bool scaled = d.nh != d.h || d.nw != d.w;
    const float scy = (float)d.h / (float)d.nh, scx = (float)d.w / (float)d.nw;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
        const int y = q / qw, x0 = (q - y * qw) << 2;
        uint32_t wi = 0, wm = 0;
        if (ok) {
            const int ry = pad_index(y - d.top, d.nh, d.border);
            const float sy = resize_coord(ry, scy, d.h);
            const int64_t my = (int64_t)(scaled ? resize_nearest(ry, scy, d.h) : ry) * d.row_stride;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int rx = pad_index(x0 + k - d.left, d.nw, d.border);
                uint8_t vi, vm;
                if (scaled) {
                    vi = sample_bilinear_strided<int64_t, true>(si, d.row_stride, d.col_stride, d.h, d.w, resize_coord(rx, scx, d.w), sy);
                    vm = sm[my + (int64_t)resize_nearest(rx, scx, d.w) * d.col_stride];
                } else {
                    vi = si[my + (int64_t)rx * d.col_stride];
                    vm = sm[my + (int64_t)rx * d.col_stride];
                }
                wi |= (uint32_t)vi << (8 * k);
                wm |= (uint32_t)vm << (8 * k);
            }
        }
        oi[q] = wi;
        om[q] = wm;
    }
}

}  // namespace

extern "C" int vs_slices_cut_u8(const uint8_t* data, int64_t data_elems, const uint8_t* labels, int64_t label_elems,
                                const vs_slice_cut* table_dev, int n, int size, uint8_t* images, uint8_t* masks, void* stream) {
    VS_REQUIRE(data && labels && table_dev && images && masks, "slices_cut_u8: null pointer");
    VS_REQUIRE(data_elems >= 1 && label_elems >= 1, "slices_cut_u8: empty volume buffer");
    VS_REQUIRE(n >= 1 && n <= 65535, "slices_cut_u8: 1 .. 65535 samples per launch, got %d", n);
    VS_REQUIRE(size >= 4 && size % 4 == 0 && size <= 16384, "slices_cut_u8: size must be a multiple of 4 in [4, 16384], got %d", size);
    VS_REQUIRE(((uintptr_t)table_dev & 7) == 0, "slices_cut_u8: the descriptor table must be 8-byte aligned");
    VS_REQUIRE(((uintptr_t)images & 3) == 0 && ((uintptr_t)masks & 3) == 0, "slices_cut_u8: outputs must be 4-byte aligned");
    const dim3 grid((unsigned)std::min(1024, cdiv(size * (size / 4), 256)), (unsigned)n);
    hipLaunchKernelGGL(slices_cut_kernel, grid, dim3(256), 0, (hipStream_t)stream, data, labels, data_elems, label_elems, table_dev, size,
                       images, masks);
    VS_LAUNCH_CHECK();
    return VS_OK;
}
