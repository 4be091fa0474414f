// Byte-image samplers shared by the training augmentations (augment.hip) and the slice feed (slice_feed.hip): cv2.remap
// semantics - bilinear in fp32 with BORDER_REFLECT_101, rounded half-to-even like np.rint.  data/augmentations.py (remap,
// resize) is the NumPy form of the same arithmetic.
#pragma once
#include "common.h"

__device__ __forceinline__ int refl101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i >= n ? period - i : i;
}

// fp32 products and sums that are each rounded on their own, as NumPy rounds them: device code is compiled with floating-point
// contraction on, and a * b + c may otherwise become one fused multiply-add (__fmul_rn / __fadd_rn do not prevent that here)
__device__ __forceinline__ float mul_unfused(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_unfused(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
// a * wa + b * wb.  EXACT: NumPy's bits.  Otherwise the compiler may fuse - the augmentations' blend, which is held to NumPy within
// a last-bit rounding on a few pixels (tests/test_augmentations.py) and whose bits stay as they are.
template <bool EXACT>
__device__ __forceinline__ float blend2(float a, float wa, float b, float wb) {
    if constexpr (EXACT) return add_unfused(mul_unfused(a, wa), mul_unfused(b, wb));
    else return __fadd_rn(__fmul_rn(a, wa), __fmul_rn(b, wb));
}

// bilinear sample of an (h x w) uint8 image at (sx, sy), reflect-101 outside, rounded half-to-even like np.rint; pixel (y, x) lives
// at img[y * rs + x * cs] (S: the index type - int for a dense image, int64_t for a slice of a volume along any axis)
template <typename S, bool EXACT>
__device__ __forceinline__ uint8_t sample_bilinear_strided(const uint8_t* img, S rs, S cs, int h, int w, float sx, float sy) {
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const S xa = refl101(x0, w) * cs, xb = refl101(x0 + 1, w) * cs, ya = refl101(y0, h) * rs, yb = refl101(y0 + 1, h) * rs;
    const float a = img[ya + xa], b = img[ya + xb], c = img[yb + xa], d = img[yb + xb];
    const float top = blend2<EXACT>(a, 1.f - fx, b, fx);
    const float bot = blend2<EXACT>(c, 1.f - fx, d, fx);
    const float v = blend2<EXACT>(top, 1.f - fy, bot, fy);
    return (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
}
__device__ __forceinline__ uint8_t sample_bilinear(const uint8_t* img, int pitch, int h, int w, float sx, float sy) {
    return sample_bilinear_strided<int, false>(img, pitch, 1, h, w, sx, sy);
}

// cv2.resize coordinates of destination index d for a source of n samples, scale = fp32(n / n_dst), in NumPy's bits:
// INTER_LINEAR: (d + 0.5) * scale - 0.5 clipped to [0, n - 1]; INTER_NEAREST: floor(d * scale), clamped
__device__ __forceinline__ float resize_coord(int d, float scale, int n) {
    return fminf(fmaxf(add_unfused(mul_unfused((float)d + 0.5f, scale), -0.5f), 0.f), (float)(n - 1));
}
__device__ __forceinline__ int resize_nearest(int d, float scale, int n) { return min((int)mul_unfused((float)d, scale), n - 1); }
